"""The C-ABI library loads and exports what include/paos_hip.h and include/paos_comm.h declare (no compute
calls without a GPU); the multi-GPU fan-out (paos_comm_* over its TCP transport, world size 2 and 3, no
torch) with a NumPy model of the device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions(name="paos_hip.h"):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(paos_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from paos_amd import _lib

    lib = _lib.load()
    names = header_functions()
    assert len(names) >= 20
    for name in names:
        assert hasattr(lib, name), f"{name} declared in include/paos_hip.h but not exported"
    assert sorted(_lib.SYMBOLS) == names, "ctypes binding table and header disagree"
    assert b"gfx950" in lib.paos_build_info()
    from paos_amd import comm

    names = header_functions("paos_comm.h")
    assert len(names) == 13
    for name in names:
        assert hasattr(lib, name), f"{name} declared in include/paos_comm.h but not exported"
    assert sorted(comm.SYMBOLS) == names, "ctypes binding table and paos_comm.h disagree"


def test_abi_struct_layout_matches_header():
    from paos_amd import _lib

    assert ctypes.sizeof(_lib.PwOp) == 12
    assert ctypes.sizeof(_lib.Pass) == 6 * 4 + 3 * _lib.MAX_PW * 12
    text = open(os.path.join(ROOT, "include", "paos_hip.h")).read()
    assert f"PAOS_MAX_PW = {_lib.MAX_PW}" in text
    assert f"PAOS_PHASE_STRIDE = {_lib.PHASE_STRIDE}" in text
    assert f"PAOS_APERTURE_STRIDE = {_lib.APERTURE_STRIDE}" in text


def test_context_creation_fails_loudly_without_gpu():
    """No CPU fallback: without a HIP device the product path raises."""
    # (not torch.cuda.is_available(): torch brings its own libamdhip64.so.7, and once it is loaded libpaoship binds to
    # that runtime instead of the one it was built against -- every GPU test later in the same process found no device)
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    from paos_amd import _lib

    with pytest.raises(_lib.PaosHipError):
        _lib.DeviceFields(64, 1)
    from paos_amd.wfo import WFO

    with pytest.raises(_lib.PaosHipError):
        WFO(1.0, 1e-6, 64, 4)


def test_context_less_error_text_is_one_per_thread_whichever_unit_fails():
    """The library is several translation units, and a failure without a context leaves its text where
    paos_last_error(NULL) reads it -- one text per thread, whichever unit raised it.  One entry point of every unit that
    has one is called with a NULL context (nothing touches a device); between two of them a call with a message of its
    own changes the text, so a unit that kept a text of its own would be caught reading the stale one.  Expected texts:
    what the library has always said -- `null context`, except for a pass program, whose one check of all its arguments
    says `bad pass program`."""
    import threading

    from paos_amd import _lib

    lib = _lib.load()
    EINVAL = 1  # include/paos_hip.h
    calls = [  # (unit, call, text)
        ("context.hip", lambda: lib.paos_sync(None), "null context"),
        ("passes.hip", lambda: lib.paos_run_passes(None, None, 0, None, 0), "bad pass program"),
        ("paos_hip.hip", lambda: lib.paos_psf_keep(None), "null context"),
        ("focus_otf.hip", lambda: lib.paos_focus_begin(None), "null context"),
        ("focus_otf.hip", lambda: lib.paos_otf_compute(None), "null context"),
        ("zoom.hip", lambda: lib.paos_zoom_compute(None, 16, 1, None, 0), "null context"),
        ("detector.hip", lambda: lib.paos_detector_add(None, None), "null context"),
    ]

    def last():
        return lib.paos_last_error(None).decode()

    def walk():
        for unit, call, text in calls:
            assert lib.paos_zoom_weights(3, 1, 0.0, None, None) == EINVAL  # (n must be even)
            assert last().startswith("paos_zoom_weights: n must be even"), (unit, last())
            assert call() == EINVAL, unit
            assert last() == text, (unit, last())

    walk()
    # ... and per thread: another thread's failures leave this thread's text alone
    assert lib.paos_zoom_weights(3, 1, 0.0, None, None) == EINVAL
    mine = last()
    errors = []

    def other():
        try:
            assert last() == ""  # nothing has failed on this thread yet
            walk()
        except AssertionError as e:  # (an assertion on another thread would otherwise only be printed)
            errors.append(e)

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert not errors, errors
    assert last() == mine


def test_shard_bounds_cover_exactly():
    from paos_amd.dist import shard_bounds

    for total in (0, 1, 7, 64, 256, 513):
        for world in (1, 2, 3, 8):
            spans = [shard_bounds(total, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1


def _spawn(target, world, *extra, timeout=300):
    import multiprocessing as mp
    import uuid

    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    key = "pytest_" + uuid.uuid4().hex
    procs = [ctx.Process(target=target, args=(r, world, key, out, *extra)) for r in range(world)]
    for p in procs:
        p.start()
    results = [out.get(timeout=timeout) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return sorted(results, key=lambda r: r[0])


def _star_worker(rank, world, key, out):
    import sys

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fakes import ModelDevice
    from paos_amd.chains import syn20_chain
    from paos_amd.comm import Comm
    from paos_amd.dist import broadcast_work, shard_bounds, syn20_work
    from paos_amd.run import _Item, _walk

    comm = Comm(world, rank, 0, "socket", key=key, timeout=120)
    try:
        total = 5
        work = syn20_work(total, "wavelengths") if rank == 0 else None
        work = broadcast_work(work, comm)
        lo, hi = shard_bounds(total, rank, world)
        wls = work["wavelengths"][lo:hi]
        chains = [syn20_chain(coefficients=c) for c in work["coefficients"][lo:hi]]
        dev = ModelDevice(64, len(chains))
        dev.fill(1.0)
        states = [_Item(1.0, wl, 64, 4, {"us": 0.0, "ut": 0.0}) for wl in wls]
        power = {}

        def on_saved(key_, items, plans, wfe):
            p = dev.norm2()
            for i, it in enumerate(items):
                power[(lo + i, it["num"])] = float(p[i])

        _walk(dev, states, chains, on_saved)
        slowest = comm.max(float(rank + 1))
        comm.barrier()
        parts = comm.allgather_scalars(np.arange(rank + 1, dtype=float) + 10 * rank)  # ragged
        text = comm.bcast_blob(b"from the last rank" if rank == world - 1 else None, root=world - 1)
        out.put((rank, lo, hi, [float(w) for w in work["wavelengths"]], power, slowest,
                 [list(p) for p in parts], text))
    finally:
        comm.close()


@pytest.mark.parametrize("world", [2, 3])
def test_comm_star_sharding(world):
    """world_size 2 and 3 on CPU over the TCP transport of paos_comm (no torch): one broadcast of the
    work description, disjoint shards that together cover the batch, MAX-reduction of the time bracket,
    ragged gather, broadcast from a non-zero root; each rank's wavefronts agree with the oracle."""
    from oracle.run_np import run as oracle_run
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.dist import shard_bounds

    results = _spawn(_star_worker, world)
    power = {}
    for rank, lo, hi, wls, pw, slowest, parts, text in results:
        assert (lo, hi) == shard_bounds(5, rank, world)
        assert wls == [syn20_wavelength(k) for k in range(5)]
        assert slowest == float(world)
        assert parts == [[10.0 * r + k for k in range(r + 1)] for r in range(world)]
        assert text == b"from the last rank"
        power.update(pw)
    assert sorted(k[0] for k in power if k[1] == 20) == [0, 1, 2, 3, 4]
    for idx in (0, 4):
        ref = oracle_run(1.0, syn20_wavelength(idx), 64, 4, {"us": 0.0, "ut": 0.0}, syn20_chain(), light=True)
        assert abs(power[(idx, 20)] - np.sum(ref[20]["amplitude"] ** 2)) < 1e-12


def _sharded_worker(rank, world, key, out, poison):
    import sys

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fakes import ModelDevice
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.comm import Comm
    from paos_amd.dist import run_sharded

    comm = Comm(world, rank, 0, "socket", key=key, timeout=120)
    try:
        total = 5
        wls = [syn20_wavelength(k * 50) for k in range(total)] if rank == 0 else None
        chains = [syn20_chain() for _ in range(total)] if rank == 0 else None
        if poison and rank == 0:
            chains[4][7]["type"] = "Hologram"  # lands in rank 1's shard; only that rank can notice
            chains[4][7]["ABCDt"] = None
        try:
            res = run_sharded(1.0, wls, 64, 4, {"us": 0.0, "ut": 0.0}, chains, batch=2, outputs=("psf",),
                              make_device=lambda n, nb: ModelDevice(n, nb), comm=comm)
        except Exception as exc:  # noqa: BLE001
            out.put((rank, "error", f"{type(exc).__name__}: {exc}"))
            return
        mine = [i for i, r in res if "psf" in r[20]]
        out.put((rank, [(i, float(r[20]["power"]), r[20]["dx"], r[20]["propagator"], r[20]["ABCDt"]().tolist())
                        for i, r in res], mine, [float(res[i][1][20]["psf"].sum()) for i in mine]))
    finally:
        comm.close()


def test_run_sharded_two_ranks():
    """run_sharded: rank 0 alone holds the work; both ranks return the full ordered list of per-wavefront
    scalars (equal on both, equal to the oracle), and each keeps the PSF arrays of its own shard only."""
    from oracle.run_np import run as oracle_run
    from paos_amd.chains import syn20_chain, syn20_wavelength

    results = _spawn(_sharded_worker, 2, False)
    (_, all0, mine0, sums0), (_, all1, mine1, sums1) = results
    assert all0 == all1
    assert [i for i, *_ in all0] == [0, 1, 2, 3, 4]
    assert mine0 == [0, 1, 2] and mine1 == [3, 4]
    for (i, power, dx, prop, abcd), psf_sum in zip([all0[0], all0[4]], [sums0[0], sums1[1]]):
        ref = oracle_run(1.0, syn20_wavelength(i * 50), 64, 4, {"us": 0.0, "ut": 0.0}, syn20_chain(), light=True)
        assert abs(power - np.sum(ref[20]["amplitude"] ** 2)) < 1e-12
        assert abs(psf_sum - np.sum(ref[20]["amplitude"] ** 2)) < 1e-12
        assert dx == ref[20]["dx"] and prop == ref[20]["propagator"]
        assert np.array_equal(np.array(abcd), ref[20]["ABCDt"]())


def test_run_sharded_failure_reaches_every_rank():
    """A chain that only rank 1 finds out it cannot run: both ranks raise, nobody hangs in the gather."""
    results = _spawn(_sharded_worker, 2, True, timeout=120)
    assert [r[1] for r in results] == ["error", "error"]
    assert "rank 1" in results[0][2] and "Hologram" not in results[0][2][:0]
    assert results[1][2]  # the failing rank re-raises its own exception


def test_wire_format_round_trip():
    """The packed work description: every type an optical chain is made of survives; nothing else packs."""
    from paos_amd import wire
    from paos_amd.abcd import ABCD
    from paos_amd.chains import parse_config_variant, syn20_chain

    chain = syn20_chain()
    back = wire.loads(wire.dumps({"wavelengths": [1.0e-6, 2.0e-6], "chains": [chain]}))
    got = back["chains"][0]
    assert list(got) == list(chain) and back["wavelengths"] == [1.0e-6, 2.0e-6]
    for k in chain:
        assert sorted(got[k]) == sorted(chain[k])
        assert np.array_equal(got[k]["ABCDt"](), chain[k]["ABCDt"]()) and got[k]["ABCDt"].cout == chain[k]["ABCDt"].cout
        assert got[k]["ABCDt"].power == chain[k]["ABCDt"].power
    assert np.array_equal(got[2]["Z"], chain[2]["Z"]) and got[2]["Zindex"].dtype == chain[2]["Zindex"].dtype
    pup, par, wls, fields, chains = parse_config_variant(os.path.join(ROOT, "data", "lens", "Ariel_AIRS-CH0.ini"))
    blob = wire.dumps(chains[0])
    assert len(blob) < 16384
    again = wire.loads(blob)
    assert list(again) == list(chains[0])
    m = np.ma.MaskedArray(np.arange(6.0).reshape(2, 3), mask=[[0, 1, 0], [0, 0, 1]])
    rt = wire.loads(wire.dumps({"m": m, "n": None, "t": (1, 2.5, "x", True), "b": b"raw"}))
    assert np.array_equal(rt["m"].mask, m.mask) and np.array_equal(rt["m"].data, m.data)
    assert rt["t"] == [1, 2.5, "x", True] and rt["n"] is None and rt["b"] == b"raw"
    with pytest.raises(TypeError):
        wire.dumps({"f": lambda: 0})
    with pytest.raises(TypeError):
        wire.dumps(np.array([object()]))
    with pytest.raises(ValueError):
        wire.loads(blob[:-3])
    with pytest.raises(ValueError):
        wire.loads(b"Zjunk")
    assert isinstance(wire.loads(wire.dumps(ABCD(thickness=1.0, curvature=0.5))), ABCD)


def test_single_rank_comm_and_bad_arguments():
    from paos_amd.comm import Comm, CommError

    c = Comm()  # one rank: no peer, no file
    assert c.max(3.5) == 3.5 and c.bcast_blob(b"abc") == b"abc"
    assert [list(p) for p in c.allgather_scalars([1.0, 2.0])] == [[1.0, 2.0]]
    c.barrier()
    c.close()
    with pytest.raises(CommError):
        Comm(2, 5, 0, "socket", key="x")
    with pytest.raises(CommError, match="key"):
        Comm(2, 1, 0, "socket", key=None, timeout=1)
    with pytest.raises(CommError, match="timed out"):
        Comm(2, 1, 0, "socket", key="nobody_listens_here", timeout=0.3)


def _fallback_worker(rank, world, key, out):
    import sys

    sys.path.insert(0, ROOT)
    from paos_amd.comm import Comm

    comm = Comm(world, rank, rank, "rccl", key=key, timeout=120)  # no GPU here: RCCL cannot come up
    try:
        text = comm.bcast_blob(b"still here" if rank == 0 else None, root=0)
        out.put((rank, comm.transport, text, comm.max(float(rank))))
    finally:
        comm.close()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a machine where RCCL cannot initialise")
def test_rccl_bring_up_failure_falls_back_to_tcp_on_every_rank():
    """Where RCCL cannot come up on every rank (here: no GPU), all ranks agree over the control plane and
    continue on the TCP transport instead of leaving each other waiting in ncclCommInitRank."""
    for rank, transport, text, slowest in _spawn(_fallback_worker, 2):
        assert transport == "socket"
        assert text == b"still here"
        assert slowest == 1.0


def _late_pair_worker(rank, world, key, out, rdv):
    import sys
    import time

    sys.path.insert(0, ROOT)
    from paos_amd.comm import Comm

    if rank == 0:
        time.sleep(1.0)  # rank 1 meets the stale file (and its unrelated listener) first
    comm = Comm(world, rank, 0, "socket", key=key, rendezvous_dir=rdv, timeout=60)
    try:
        out.put((rank, comm.bcast_blob(b"fresh" if rank == 0 else None, root=0), comm.max(float(rank))))
    finally:
        comm.close()


def test_stale_rendezvous_file_and_stray_connections_are_not_trusted(tmp_path):
    """A rendezvous file left behind by a dead job may name a port that now belongs to somebody else: a peer
    that connects there gets no valid handshake and keeps looking until rank 0 of ITS job has published the
    real port.  A stranger connecting to rank 0's port (and saying nothing) does not stall or fail rank 0."""
    import multiprocessing as mp
    import socket
    import threading
    import uuid

    key = "pytest_" + uuid.uuid4().hex
    stranger = socket.socket()
    stranger.bind(("127.0.0.1", 0))
    stranger.listen(8)
    stale_port = stranger.getsockname()[1]
    (tmp_path / f"paos_comm_{key}").write_text(f"{stale_port}\n")
    stop = threading.Event()
    visits = []

    def serve():  # accepts, answers with junk, hangs up
        stranger.settimeout(0.2)
        while not stop.is_set():
            try:
                conn, _ = stranger.accept()
            except OSError:
                continue
            visits.append(1)
            try:
                conn.sendall(b"\x00" * 16)
            finally:
                conn.close()

    th = threading.Thread(target=serve, daemon=True)
    th.start()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_late_pair_worker, args=(r, 2, key, out, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()

    def poke():  # while rank 0 waits for its peer: connect to whatever port the file names now, say nothing
        import time

        for _ in range(200):
            try:
                port = int((tmp_path / f"paos_comm_{key}").read_text())
            except (OSError, ValueError):
                time.sleep(0.01)
                continue
            if port != stale_port:
                try:
                    s = socket.create_connection(("127.0.0.1", port), timeout=1)
                    time.sleep(0.5)
                    s.close()
                except OSError:
                    pass
                return
            time.sleep(0.01)

    pk = threading.Thread(target=poke, daemon=True)
    pk.start()
    results = sorted(out.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    stop.set()
    th.join(timeout=5)
    stranger.close()
    assert visits, "rank 1 never met the stale port: the test did not exercise the handshake"
    assert results == [(0, b"fresh", 1.0), (1, b"fresh", 1.0)]


def test_from_env_wants_a_job_key(monkeypatch):
    from paos_amd.comm import Comm, CommError

    for name in ("PAOS_COMM_KEY", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    with pytest.raises(CommError, match="PAOS_COMM_KEY"):
        Comm.from_env(transport="socket", timeout=1)


def test_model_device_keeps_the_psf():
    """run_batch(keep_psf=True) on the NumPy model of the device: the PSF of the last surface is what
    psf_fetch returns (the model mirrors paos_psf_keep / paos_psf_keep_power)."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fakes import ModelDevice
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    wls = [syn20_wavelength(0), syn20_wavelength(200)]
    for power in (True, False):
        dev = ModelDevice(64, 2)
        res = run_batch(1.0, wls, 64, 4, {"us": 0.0, "ut": 0.0}, [syn20_chain(), syn20_chain()], outputs=("psf",),
                        dev=dev, keep_psf=True, power=power)
        for i in range(2):
            assert np.array_equal(dev.psf_fetch(i), res[i][20]["psf"])
            if power:
                assert abs(res[i][20]["power"] - res[i][20]["psf"].sum()) < 1e-13


def test_bench_self_launch_starts_ranks_relays_rank0_and_propagates_failure(capfd):
    """VERDICT r03 "next" 2: `python bench.py --gpus N` with no launcher starts its own N ranks (fresh processes with
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* and a job key), relays rank 0's JSON line and returns non-zero when any
    rank did.  Exercised here with stand-in ranks on the library's TCP transport (tests/bench_rank_stub.py: join,
    broadcast, barrier, MAX, gather); the real bench.py runs through the same launcher on the GPU box
    (tests/test_gpu_r3.py::test_bench_two_self_launched_ranks_on_one_gpu)."""
    import json
    import sys

    sys.path.insert(0, ROOT)
    import bench

    stub = [sys.executable, os.path.join(ROOT, "tests", "bench_rank_stub.py")]
    for world in (2, 3):
        rc = bench.self_launch(world, [], child=stub, timeout=120.0)
        out = capfd.readouterr().out.strip().splitlines()
        assert rc == 0 and len(out) == 1, out
        line = json.loads(out[0])
        assert line["n_gpus"] == world and line["devices_seen"] == list(range(world)) and line["shard"] == [0, 4]
        assert line["ipc"] == "0" and line["self_launched"] == "1" and line["key"].startswith("bench_")
        assert abs(line["value"] - 4 * world / (0.001 * world)) < 1e-6  # MAX over the ranks' brackets
    # a rank that dies: the launcher reports its exit code; the others time out at the rendezvous and are reaped
    rc = bench.self_launch(2, [], child=stub, timeout=60.0, env_extra={"STUB_FAIL_RANK": "1"}, grace=2.0)
    assert rc == 7
    # one GPU shared by every rank (the rehearsal switch): LOCAL_RANK is 0 everywhere
    os.environ["PAOS_BENCH_REHEARSAL"] = "1"
    try:
        rc = bench.self_launch(2, [], child=stub, timeout=120.0)
    finally:
        del os.environ["PAOS_BENCH_REHEARSAL"]
    line = json.loads(capfd.readouterr().out.strip().splitlines()[-1])
    assert rc == 0 and line["devices_seen"] == [0, 0]


def test_bench_roofline_block_accounting():
    """bench.py's roofline block from synthetic launch records: `achieved` over every launch on the plan's bytes, `dense`
    from the un-pruned leg, classes cut into steps by the launches timed per step (a launch may run two or three passes),
    counter bytes and vector instructions matched by launch order.  Pure host logic: no GPU, no library."""
    import numpy as np

    import bench

    class Dev:
        def copy_yardstick(self, reps):
            return 3.0, 2 * 16 * 4096 * 4096 * 32

    steps, per_step = 2, 3
    ms = np.array([1.0, 2.0, 0.5, 1.0, 2.0, 0.5])
    tags = np.array([1 | 2, 1 | 2 | 4 | 16, 1 | 8 | 32] * steps, dtype=np.int32)
    planned = np.array([2.0e9, 1.0e9, 1.0e9] * steps)
    m = {"launch_ms": ms, "launch_tags": tags, "launch_bytes": planned, "fused_passes": 6, "per_step_passes": [6, 6],
         "per_step_launches": [per_step, per_step], "first_timed_step": 3}
    dense = {"launch_ms": np.array([4.0, 4.0, 1.0]), "launch_tags": np.array([0, 0, 8], dtype=np.int32)}
    traffic = {"pass": [(1.2e9, 1.0e9), (0.6e9, 0.6e9), (0.5e9, 0.7e9)], "other": {}, "pass_valu": [4.0e8, 8.0e8, 2.0e8]}
    n, nb, esz = 4096, 32, 16
    r = bench.roofline_block(m, n, nb, esz, Dev(), "k", steps, traffic, dense=dense)
    full = 2 * esz * n * n * nb
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s"
    assert abs(r["achieved"] - planned.sum() / (ms.sum() * 1e-3) / 1e9) < 1e-9
    assert abs(r["frac"] - r["achieved"] / 8000.0) < 1e-12
    assert r["launches"] == 6 and r["launches_per_step"] == 3.0 and r["full_pass_bytes"] == full
    assert abs(r["dense"]["achieved"] - full / 4.0e-3 / 1e9) < 1e-6 and r["dense"]["launches"] == 2
    assert len(r["classes"]) == 3
    two = [v for k, v in r["classes"].items() if "two passes" in k][0]
    assert two["launches_per_step"] == 1.0 and two["avg_launch_ms"] == 2.0 and two["bytes_planned"] == 1.0e9 and two["bytes_measured"] == 1.2e9
    assert abs(r["traffic"] - (2.2e9 + 1.2e9 + 1.2e9) / 3) < 1.0
    assert abs(r["traffic_over_algorithmic"] - 4.6e9 / 4.0e9) < 1e-12
    assert abs(r["issue"]["frac_of_issue_peak"] - (1.4e9 * 4 / 1024) / (3.5e-3 * 2.4e9)) < 1e-12
    # without counters and without a dense leg the block still stands
    r2 = bench.roofline_block(m, n, nb, esz, Dev(), "k", steps)
    assert r2["traffic"] is None and "dense" not in r2 and "issue" not in r2 and len(r2["classes"]) == 3


def test_bench_contract_line_is_small_strict_json():
    """The ONE line bench.py prints (a 25 KB line did not parse): built from a synthetic measure() result with the
    worst-case texts, it stays under 4 KB, round-trips as strict JSON (no NaN / Infinity), carries `roofline` and
    `cpu_baseline` with the contract's keys, names the bound by the larger of the two roofline fractions of the dominant
    class of launch, and the detail record is strict JSON too.  Pure host logic."""
    import json

    import numpy as np

    import bench

    class Dev:
        def copy_yardstick(self, reps):
            return 3.0, 2 * 16 * 4096 * 4096 * 32

    steps, n, nb, esz = 2, 4096, 32, 16
    ms = np.array([0.8, 1.3, 1.3, 0.9] * steps)
    tags = np.array([1 | 4, 1 | 2 | 4 | 16, 1 | 2 | 4 | 16, 1 | 8 | 32] * steps, dtype=np.int32)
    planned = np.array([2.7e9, 1.09e9, 1.09e9, 0.89e9] * steps)
    lines = np.array([2 * 33024.0, 4 * 33024.0, 4 * 33024.0, 5 * 33024.0] * steps)
    m = {"launch_ms": ms, "launch_tags": tags, "launch_bytes": planned, "launch_lines": lines, "fused_passes": 24,
         "per_step_passes": [24, 24], "per_step_launches": [4, 4], "first_timed_step": 1}
    traffic = {"pass": [(1.4e9, 1.4e9), (0.8e9, 0.62e9), (0.8e9, 0.62e9), (0.9e9, 0.66e9)], "other": {},
               "pass_valu": [2.2e8, 4.7e8, 4.7e8, 4.2e8]}
    dense = {"launch_ms": np.array([3.8, 3.9]), "launch_tags": np.array([0, 0], dtype=np.int32)}
    dom = bench.dominant_launch(m, n, "fp64", steps, traffic)
    assert dom["tag"] == (1 | 2 | 4 | 16) and dom["launches"] == 4 and abs(dom["avg_launch_ms"] - 1.3) < 1e-12
    flops = 4 * 33024.0 * 5 * 4096 * 12
    assert abs(dom["TFLOPs"] - flops / 1.3e-3 / 1e12) < 1e-9 and abs(dom["flop_frac"] - dom["TFLOPs"] / 78.6) < 1e-12
    assert abs(dom["hbm_frac"] - 1.09e9 / 1.3e-3 / 1e9 / 8000.0) < 1e-12
    assert abs(dom["issue_frac"] - (4.7e8 * 4 / 1024) / (1.3e-3 * 2.4e9)) < 1e-12
    assert abs(dom["traffic"] - 1.42e9) < 1.0 and abs(dom["traffic_over_planned"] - 1.42e9 / 1.09e9) < 1e-12
    assert dom["bound"] == "valu_fp64"  # 0.57 of the issue slots against 0.10 (0.14 on counted bytes) of 8 TB/s
    full = {
        "metric": "wavefronts/sec (4096^2 c128, 20-surface chain) + achieved HBM GB/s", "value": 1987.123456789, "unit": "wavefronts/s",
        "n_gpus": 1, "steps": steps, "warmup": 3, "ms_per_step": 16.1234567, "dtype": "c128 (f64)",
        "config": {"workload": "w" * 2000, "workload_notes": "x" * 5000, "grid": n, "batch_per_gpu": nb,
                   "parallelism": "wavefront-sharded x1", "transport": "none (single process)", "launcher": "none",
                   "ranks_seen": 1, "devices_seen": [0], "bringup_notes": {"0": "y" * 3000}},
        "roofline": bench.roofline_block(m, n, nb, esz, Dev(), "frugal_pass_kernel (every FFT pass launch, rows and columns)", steps,
                                         traffic, dense=dense),
        "dominant_launch": dom,
        "ptp_step": {"frac_bytes_moved": 0.636, "ms_per_wavefront": float("nan")},
        "extra": {"big": ["z" * 100] * 300, "inf": float("inf"), "arr": np.arange(4), "np": np.float64(1.5),
                  "2048^2": {"value": np.float64(6990.123456), "unit": "wavefronts/s", "roofline": {"w": "v" * 4000}},
                  "dense": {"value": float("nan"), "unit": "wavefronts/s"}, "broken": {"error": "e" * 3000},
                  "psd_screen": {"device_ms": 31.23456, "host_ms": 2950.5, "what": "p" * 500}},
        "cpu_baseline": {"value": 0.0213, "unit": "wavefronts/s", "cores": 1, "kind": "port", "sample": "s" * 1000},
        "detail_file": "bench_detail.json",
    }
    text = bench.contract_line(full)
    assert len(text) < 4096 and "\n" not in text
    brief = json.loads(text)["extra_wavefronts_per_s"]  # one number per side measurement, nothing else of them
    assert brief == {"2048^2": 6990.0, "dense": None, "psd_screen_ms": {"device": 31.23, "host": 2950.0}}, brief  # (4 significant digits)
    line = json.loads(text, parse_constant=lambda c: (_ for _ in ()).throw(ValueError(c)))  # NaN / Infinity would raise
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["value"] == 1987.12 and line["higher_is_better"] is True and line["vs_baseline"] is None
    r = line["roofline"]
    for key in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch",
                "avg_launch_ms", "launches", "hbm_frac", "flop_frac", "issue_frac", "traffic_over_planned", "dense_frac",
                "ptp_step_frac", "all_launches_hbm_frac", "copy_yardstick_frac"):
        assert key in r, key
    assert r["bound"] == "valu_fp64" and r["unit"] == "TFLOP/s" and r["peak"] == 78.6
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 2e-3 and r["ptp_step_frac"] == 0.636
    assert abs(r["dense_frac"] - 2 * esz * n * n * nb / 3.85e-3 / 1e9 / 8000.0) < 1e-3
    assert len(line["config"]["workload"]) <= 300 and set(line["cpu_baseline"]) == {"value", "unit", "cores", "kind", "sample"}
    # an hbm-bound dominant class names hbm and reports GB/s
    m2 = dict(m, launch_bytes=planned * 8.0)
    full2 = dict(full, dominant_launch=bench.dominant_launch(m2, n, "fp64", steps, None))
    l2 = json.loads(bench.contract_line(full2))
    assert l2["roofline"]["bound"] == "hbm" and l2["roofline"]["unit"] == "GB/s" and l2["roofline"]["peak"] == 8000.0
    # the exit-3 record of a scaling run without RCCL: same function, value null
    l3 = json.loads(bench.contract_line({"metric": "m", "value": None, "unit": "wavefronts/s", "n_gpus": 8, "steps": 5, "warmup": 1,
                                         "ms_per_step": None, "dtype": "c128 (f64)", "error": "e" * 1000,
                                         "config": {"workload": "not run", "ranks_seen": 8, "devices_seen": list(range(8))}}))
    assert l3["value"] is None and l3["config"]["ranks_seen"] == 8 and len(l3["error"]) <= 800
    # the detail record: strict JSON whatever the measurements held
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        path = bench.write_detail(full, os.path.join(tmp, "d.json"))
        back = json.load(open(path), parse_constant=lambda c: (_ for _ in ()).throw(ValueError(c)))
        assert back["extra"]["inf"] is None and back["extra"]["arr"] == [0, 1, 2, 3] and back["ptp_step"]["ms_per_wavefront"] is None


def test_dmabuf_ipc_is_exported_only_for_an_rccl_communicator():
    """importing paos_amd.comm (or opening a TCP communicator) leaves HSA_ENABLE_IPC_MODE_LEGACY alone; asking
    for RCCL exports it (before the library makes its first HIP call), keeps a value the user set, and warns when the
    process has already created a device context."""
    import subprocess
    import sys
    import textwrap

    code = textwrap.dedent("""
        import os, sys, warnings
        os.environ.pop("HSA_ENABLE_IPC_MODE_LEGACY", None)
        sys.path.insert(0, %r)
        from paos_amd import _lib, comm
        assert "HSA_ENABLE_IPC_MODE_LEGACY" not in os.environ, "import exported it"
        c = comm.Comm(1, 0, 0, "socket", key="ipc_test_%%d" %% os.getpid())
        c.close()
        assert "HSA_ENABLE_IPC_MODE_LEGACY" not in os.environ, "a TCP communicator exported it"
        comm._want_dmabuf_ipc()
        assert os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
        os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "1"
        comm._want_dmabuf_ipc()
        assert os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] == "1", "the user's value was overwritten"
        del os.environ["HSA_ENABLE_IPC_MODE_LEGACY"]
        _lib._HIP_TOUCHED[0] = True
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            comm._want_dmabuf_ipc()
        assert len(w) == 1 and "already used the GPU" in str(w[0].message), w
        print("ok")
    """) % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr


def test_bench_finds_the_counted_step_of_a_pmc_child_run():
    """bench.measure_traffic keeps the dispatches of the LAST step of its child runs (a warm-up step, then the counted one).
    Since round 5 the start's power kernel runs only when the sums are not found from the step before, so a step is
    recognised by the kernel that writes the start field -- with the power kernel and its reduction in front when present."""
    import bench

    power = ["void paos::start_power_kernel<double, 4, 2, 0>(...)", "paos::norm2_final_kernel(...)"]
    body = ["void paos::start_write_kernel<double, 4, 2, 0>(...)", "void paos::norm2_partial_kernel<double>(...)",
            "paos::norm2_final_kernel(...)", "void paos::zernike_kernel<double, 4, 2, 8>(...)",
            "void paos::frugal_pass_kernel<double, 4096, ...>(...)", "void paos::mask_lines_kernel<0>(...)"]
    assert bench.counted_step_from(power + body + body) == len(power) + len(body)           # sums found on the second step
    assert bench.counted_step_from(power + body + power + body) == len(power) + len(body)   # PAOS_START_POWER_MEMO=0
    assert bench.counted_step_from(body) == 0 and bench.counted_step_from(power + body) == 0
    assert bench.counted_step_from(["void paos::frugal_pass_kernel<...>(...)"]) == 0        # (a chain without a start: everything)


def test_bench_measure_arms_the_launch_timer_in_front_of_the_warm_up():
    """bench.measure: the launch timer's events are created BEFORE the warm-up steps and the timer is re-armed behind them --
    creating them behind the warm-up left the GPU idle for the better part of a second in front of the timed region (round 5:
    20 timed steps measured 1.7 % under 400).  On the NumPy model of the device: the order of calls, exactly K timed steps
    behind W warm-up steps, one walked block of wavelengths per step."""
    import numpy as np

    import bench
    from fakes import ModelDevice
    from paos_amd.chains import syn20_chain, syn20_wavelength

    calls = []

    class Timed(ModelDevice):
        def profile_begin(self, kind, max_launches=0):
            calls.append(("profile_begin", max_launches))

        def profile_planned_bytes(self):
            return np.zeros(0)

        def profile_line_transforms(self):
            return np.zeros(0)

        def profile_end_launches(self):
            return np.zeros(0), np.zeros(0, dtype=np.int32)

        def start(self, *a, **k):
            calls.append(("step", None))
            return super().start(*a, **k)

        def sync(self):
            calls.append(("sync", None))
            return super().sync()

    n, nb, steps, warmup = 64, 2, 3, 2
    seen = []

    def wavelengths_of(g):
        seen.append(g)
        return [syn20_wavelength((g * nb + i) % 512) for i in range(nb)]

    m = bench.measure(Timed(n, nb), n, "fp64", wavelengths_of, [syn20_chain() for _ in range(nb)], steps, warmup)
    kinds = [k for k, _ in calls]
    first, second = [i for i, k in enumerate(kinds) if k == "profile_begin"]
    assert kinds[:first].count("step") == 0                      # the events exist before anything runs
    assert kinds[first:second].count("step") == warmup and "sync" in kinds[first:second]
    assert kinds[second:].count("step") == steps and kinds[-1] == "sync"
    assert calls[first][1] == calls[second][1] >= 24 * steps     # re-armed with the same capacity: nothing is created then
    assert seen == list(range(warmup + steps)) and m["elapsed"] > 0 and len(m["per_step_passes"]) == steps


def test_bench_dump_outputs_writes_the_last_step_within_its_budget(tmp_path):
    """bench.py --dump-outputs: the last timed step's records and kept PSFs as float64 .npy files, under 64 MB in all
    (dump_shape: a central crop and a seeded pixel sample of every PSF), the same files for the same step every time.
    On the NumPy model of the device: the crop and the sample are the PSF's own pixels, the last surface's power is the
    PSF's sum, and asking for zero timed steps is refused."""
    import bench
    from fakes import ModelDevice
    from paos_amd.chains import syn20_chain, syn20_wavelength

    for n, nb in ((4096, 32), (4096, 1), (2048, 128), (1024, 512), (256, 4096)):
        c, s = bench.dump_shape(n, nb)
        assert 0 < c <= min(n, 256) and 0 < s <= n * n and 8 * nb * (c * c + s) + 4096 <= bench.DUMP_LIMIT
    assert bench.dump_shape(4096, 32) == (256, 168823)  # the flagship: 32 PSFs of 4096^2

    n, nb = 64, 2
    chains = [syn20_chain() for _ in range(nb)]

    def wavelengths_of(g):
        return [syn20_wavelength((g * nb + i) % 512) for i in range(nb)]

    dirs = []
    for k in range(2):
        dev = ModelDevice(n, nb)
        m = bench.measure(dev, n, "fp64", wavelengths_of, chains, 2, 1, timer=False, keep_last=True)
        dirs.append(str(tmp_path / f"run{k}"))
        written = bench.dump_outputs(dev, m["res"], dirs[-1])
        assert 0 < written <= bench.DUMP_LIMIT
    c, s = bench.dump_shape(n, nb, np.load(os.path.join(dirs[0], "records.npy")).nbytes)
    got = {name: np.load(os.path.join(dirs[0], name + ".npy")) for name in ("records", "psf_centre", "psf_sample")}
    for name, arr in got.items():
        assert arr.dtype == np.float64 and np.isfinite(arr).all(), name
        assert np.array_equal(arr, np.load(os.path.join(dirs[1], name + ".npy"))), name
    assert got["psf_centre"].shape == (nb, c, c) and got["psf_sample"].shape == (nb, s)
    records = got["records"]
    assert records.shape[0] == nb and list(records[:, 0]) == list(range(nb)) and (records[:, 1] == 2).all()
    pixels = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, n * n, s))
    lo = (n - c) // 2
    for i in range(nb):
        psf = dev.psf_fetch(i)
        assert np.array_equal(got["psf_centre"][i], psf[lo:lo + c, lo:lo + c])
        assert np.array_equal(got["psf_sample"][i], psf.ravel()[pixels])
        assert records[i, 2 + 26] == 20 and abs(records[i, 2 + 26 + 12] - psf.sum()) <= 1e-12 * psf.sum()
        assert records[i, 2 + 6] == 0.0  # 1 / f-ratio behind the stop: the beam is collimated there (f-ratio inf)
        assert records[i, 2 + 26 + 6] == 1.0 / m["res"][i][20]["fratio"]
    with pytest.raises(SystemExit):
        bench.main(["--steps", "0"])


def test_bench_plain_run_measures_the_headline_only_and_full_runs_the_rest(tmp_path, monkeypatch, capsys):
    """bench.py without --full: set-up, warm-up, the timed steps and the line -- no CPU baseline, no counter children, no
    side measurement on the context, no copy yardstick, no detail file unless --detail names one.  With --full all of them
    run and land in the line and the detail record.  On the NumPy model of the device (grid 64: no `extra` entries), with
    the CPU baselines and the counter children replaced by stand-ins that record their calls."""
    import json

    import bench
    from fakes import ModelDevice
    from paos_amd import _lib

    calls = []

    class Device(ModelDevice):
        def profile_begin(self, kind, max_launches=0):
            pass

        def profile_end(self):
            return 3, 1.5

        def profile_planned_bytes(self):
            return np.zeros(0)

        def profile_line_transforms(self):
            return np.zeros(0)

        def profile_end_launches(self):
            return np.zeros(0), np.zeros(0, dtype=np.int32)

        def copy_yardstick(self, reps=10):
            calls.append("copy_yardstick")
            return 1.0, 8.0e9

        def ptp(self, blocks):
            calls.append("ptp")
            return super().ptp(blocks)

    for key in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "PAOS_BENCH_FORCE_COMM"):
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setattr(_lib, "DeviceFields", Device)
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))  # where --full puts bench_detail.json by default
    monkeypatch.setattr(bench, "cpu_baseline_parallel", lambda n, nb: calls.append("cpu_parallel") or {"value": 2.0})
    monkeypatch.setattr(bench, "cpu_baseline", lambda n: calls.append("cpu_single") or
                        {"value": 1.0, "unit": "wavefronts/s", "cores": 1, "kind": "port", "sample": "s"})
    monkeypatch.setattr(bench, "measure_traffic", lambda *a: calls.append("traffic") or (None, "stand-in"))
    small = ["--grid", "64", "--batch", "2", "--steps", "2", "--warmup", "1"]

    bench.main(small)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert calls == [] and os.listdir(tmp_path) == []
    assert line["value"] > 0 and line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "wavefronts/s" and line["higher_is_better"] is True and line["dtype"] == "c128 (f64)"
    assert line["cpu_baseline"] is None and line["detail"] is None and "extra_wavefronts_per_s" not in line
    assert line["roofline"]["ptp_step_frac"] is None and line["roofline"]["copy_yardstick_frac"] is None

    detail = str(tmp_path / "plain.json")
    bench.main(small + ["--detail", detail])
    capsys.readouterr()
    rec = json.load(open(detail))
    assert calls == [] and rec["sweep"]["walked"] is True and rec["ptp_step"] is None
    assert rec["without_ptp_algebra"] is None and rec["same_wavelengths_every_step"] is None
    assert rec["roofline"]["copy_yardstick"] is None and "dense" not in rec["roofline"] and "cpu_baseline" not in rec
    os.remove(detail)

    bench.main(small + ["--full"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert calls[:2] == ["cpu_parallel", "traffic"] and calls[-1] == "cpu_single"
    assert "ptp" in calls and "copy_yardstick" in calls
    assert line["value"] > 0 and line["cpu_baseline"]["value"] == 1.0 and line["detail"] == "bench_detail.json"
    rec = json.load(open(tmp_path / "bench_detail.json"))
    assert rec["ptp_step"]["ms_per_wavefront"] == 0.3 / 2 and rec["cpu_baseline_parallel"] == {"value": 2.0}
    assert rec["without_ptp_algebra"]["steps"] == 2 and rec["operator_by_operator"]["steps"] == 2
    assert rec["same_wavelengths_every_step"]["value"] > 0 and rec["roofline"]["copy_yardstick"]["GBps"] == 8000.0
    assert rec["roofline"]["counters_note"] == "stand-in"
