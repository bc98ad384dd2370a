"""The sweep of tests/test_gpu_upload_batches.py: shared by the test (the references, one fresh context per checked step) and
by the fresh processes it starts for the switches the library reads once per process or per context (PAOS_ARENA_DOUBLES,
PAOS_STAGE_PROGRAM, PAOS_BATCHED_RECORDS, PAOS_DUMP_PASSES).  The sweep marks every step on stderr ("sweep step G") between
the library's own lines."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NB, STEPS = 1024, 3, 40  # the smallest grid of the production pass kernels, batch 3
ON_AXIS = {"us": 0.0, "ut": 0.0}
# The steps whose results are read (a read synchronises; in between the host runs ahead of the GPU, as in bench.measure): the
# first two, then one in seven -- with the slab the test asks for every step switches slabs at least once, so each stretch
# in between goes round all four slabs more than once -- and the last.
CHECKED = (0, 1, 2, 9, 16, 23, 30, 37, STEPS - 1)
SLAB_DOUBLES = 2048  # PAOS_ARENA_DOUBLES of the sweeps: the first program grows the slabs to what one program needs


def wavelengths_of(g):
    from paos_amd.chains import syn20_wavelength

    return [syn20_wavelength((g * NB + i) % 512) for i in range(NB)]


def lean_step(dev, g, chains):
    """bench.measure's call for step g: nothing waits, the PSFs stay on the device, the powers are tickets."""
    from paos_amd.run import run_batch

    return run_batch(1.0, wavelengths_of(g), N, 4, ON_AXIS, chains, outputs=(), dev=dev, sync=False, keep_psf=True)


def tickets(res):
    return list({id(rec["power_ticket"]): rec["power_ticket"] for r in res for rec in r.values() if "power_ticket" in rec}.values())


def read_step(dev, res):
    """What is compared: per item the digest of the PSF's bytes and the bits of every saved surface's power."""
    import numpy as np

    out = {"psf": [], "power": []}
    for i in range(NB):
        out["power"].append({str(k): float(rec["power_ticket"].fetch()[i]).hex() for k, rec in sorted(res[i].items()) if "power_ticket" in rec})
    for i in range(NB):
        psf = dev.psf_fetch(i)
        assert np.isfinite(psf).all() and psf.max() > 0.0
        out["psf"].append(hashlib.sha256(np.ascontiguousarray(psf).tobytes()).hexdigest())
    return out


def step_alone(g):
    """Step g on a fresh context (the library's defaults)."""
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain

    dev = _lib.DeviceFields(N, NB)
    try:
        return read_step(dev, lean_step(dev, g, [syn20_chain() for _ in range(NB)]))
    finally:
        dev.close()


def sweep():
    """STEPS consecutive steps on one context; {step: read_step} for the CHECKED ones."""
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain

    chains = [syn20_chain() for _ in range(NB)]
    dev = _lib.DeviceFields(N, NB)
    got, res = {}, None
    try:
        for g in range(STEPS):
            sys.stderr.write(f"sweep step {g}\n")
            sys.stderr.flush()
            if res is not None:  # the tickets of a step nobody reads go back unread (no synchronisation)
                for t in tickets(res):
                    t.release()
            res = lean_step(dev, g, chains)
            if g in CHECKED:
                got[str(g)] = read_step(dev, res)
    finally:
        dev.close()
    return got


def sweep_worker(out, env):
    """In a fresh process: the sweep under the switches ``env``, with the process's stderr in a file.  Puts ("ok", results,
    slab switches per step) or ("fail", message) on ``out``."""
    import tempfile

    try:
        os.environ.update(env)
        with tempfile.TemporaryFile(mode="w+") as log:
            keep = os.dup(2)
            os.dup2(log.fileno(), 2)
            try:
                got = sweep()
            finally:
                sys.stderr.flush()
                os.dup2(keep, 2)
                os.close(keep)
            log.seek(0)
            switches, step = {}, None
            for line in log:
                if line.startswith("sweep step "):
                    step = int(line.split()[2])
                    switches[step] = 0
                elif line.startswith("arena switch") and step is not None:
                    switches[step] += 1
        out.put(("ok", got, switches))
    except Exception as exc:  # noqa: BLE001 -- the parent reports it
        out.put(("fail", repr(exc), None))
