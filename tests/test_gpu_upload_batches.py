"""GPU test of the batched parameter uploads (csrc/context.hip: ArenaBatch): every block a call adds in front of its first
launch travels in one copy, and the device pointers go to kernels behind that copy only.  A launch in front of its copy
would read what the slab held four switches ago and nothing would report it -- except results that differ from those of a
context that has no history.  So: a walked lean SYN20 sweep of 40 consecutive steps on ONE context, another block of
wavelengths every step, issued as bench.measure issues them (nothing waits, the PSFs stay on the device), on slabs so small
(PAOS_ARENA_DOUBLES) that every step leaves its slab; the PSFs and the powers of the saved surfaces of the checked steps
against a fresh context that runs that step alone, bit for bit.  Each sweep runs in a fresh process (the switches are read
once per process), with PAOS_DUMP_PASSES=1, whose lines say where the slabs were switched.

Which steps are checked (tests/upload_batches_worker.py: CHECKED): a read synchronises, and a sweep that is read at every
step never runs ahead of the GPU, which is when a slab is refilled while its last readers are still queued.  So the first
three steps are read (the steps behind the first switches), then one step in seven, then the last; the test asserts from
the dump that every step switched slabs at least once -- every checked step is a step behind a switch -- and that each
unread stretch went round all four slabs."""
import pytest

import upload_batches_worker as worker

pytestmark = pytest.mark.gpu

SLABS = 4  # kArenaSlabs


@pytest.fixture(scope="module")
def alone():
    """{step: results} of every checked step on a context of its own: computed once, shared by the three sweeps."""
    return {str(g): worker.step_alone(g) for g in worker.CHECKED}


def run_sweep(switch=None):
    import multiprocessing as mp

    env = {"PAOS_ARENA_DOUBLES": str(worker.SLAB_DOUBLES), "PAOS_DUMP_PASSES": "1"}
    if switch:
        env[switch] = "0"
    ctx = mp.get_context("forkserver")  # (the server conftest.py started before this process touched the GPU)
    out = ctx.Queue()
    proc = ctx.Process(target=worker.sweep_worker, args=(out, env))
    proc.start()
    try:
        status, got, switches = out.get(timeout=300)
        proc.join(timeout=60)
    finally:
        if proc.is_alive():  # (a worker that hangs must not stay behind with the GPU open)
            proc.kill()
    assert status == "ok", got
    return got, switches


@pytest.mark.parametrize("switch", [None, "PAOS_STAGE_PROGRAM", "PAOS_BATCHED_RECORDS"])
def test_a_sweep_on_small_slabs_equals_fresh_contexts(alone, switch):
    """The default path (one copy per program and per start) and the two that stage launch by launch (PAOS_STAGE_PROGRAM=0:
    item records and tables per launch; PAOS_BATCHED_RECORDS=0: aperture records rendered in place, one vector per push)."""
    got, switches = run_sweep(switch)
    assert sorted(got, key=int) == [str(g) for g in worker.CHECKED]
    assert sorted(switches) == list(range(worker.STEPS))
    print("slab switches per step:", [switches[g] for g in range(worker.STEPS)])
    assert all(switches[g] >= 1 for g in range(1, worker.STEPS)), switches  # every step leaves its slab
    # the unread stretches of seven steps go round every slab, the GPU behind the host (the last step follows a read closely)
    for a, b in zip(worker.CHECKED[2:-1], worker.CHECKED[3:-1]):
        assert sum(switches[g] for g in range(a + 1, b + 1)) > SLABS, (a, b)
    for g in worker.CHECKED:
        for i in range(worker.NB):
            assert got[str(g)]["power"][i] == alone[str(g)]["power"][i], (g, i, got[str(g)]["power"][i], alone[str(g)]["power"][i])
            assert len(got[str(g)]["power"][i]) >= 2  # the first surface (the start field's own power) and the image plane
            assert got[str(g)]["psf"][i] == alone[str(g)]["psf"][i], (g, i)
    psfs = [got[str(g)]["psf"][0] for g in worker.CHECKED]
    assert len(set(psfs)) == len(psfs)  # (the steps do differ)
