"""The N > 1 path on CPU: PRN / channel shard planner and the acquisition peak gather over
torch.distributed (gloo, world_size 2, rendezvous on 127.0.0.1)."""
import importlib
import os
import socket
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, pkg


def test_plan_shards_is_a_balanced_partition():
    sh = pkg("shard")
    for n, w in ((32, 1), (32, 2), (32, 8), (32, 5), (8, 8), (3, 8), (64, 8)):
        parts = sh.plan_shards(n, w)
        assert len(parts) == w
        flat = [i for r in parts for i in r]
        assert flat == list(range(n))
        sizes = [len(r) for r in parts]
        assert max(sizes) - min(sizes) <= 1
    assert [len(r) for r in sh.plan_shards(32, 8)] == [4] * 8       # BASELINE.json config 4: 4 PRN / GPU
    assert [len(r) for r in sh.plan_shards(64, 8)] == [8] * 8       # config 5: 8 channels / GPU
    with pytest.raises(ValueError):
        sh.plan_shards(4, 0)


def test_pack_merge_roundtrip_reproduces_single_gpu_arrays():
    sh = pkg("shard")
    g = load_golden("acq_default.npz")
    full = dict(carrFreq=g["carrFreq"], codePhase=g["codePhase"], peakMetric=g["peakMetric"],
                freqBin=g["freqBin"], fineIdx=g["fineIdx"])
    for world in (1, 2, 8, 5):
        bufs = []
        slots = -(-32 // world)
        for r in range(world):
            mine = list(sh.plan_shards(32, world)[r])
            res = {k: v[mine] for k, v in full.items()}
            bufs.append(sh.pack_peaks(mine, res, slots))
        m = sh.merge_peaks(np.stack(bufs))
        for k in ("carrFreq", "codePhase", "peakMetric", "freqBin"):
            assert np.array_equal(m[k], full[k]), (world, k)
        det = full["carrFreq"] > 0
        assert np.array_equal(m["fineIdx"][det], full["fineIdx"][det])
    assert sh.PEAK_DTYPE.itemsize == 40


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sh = importlib.import_module("softgnss-python_amd.shard")
        g = np.load(os.path.join(ROOT, "tests", "golden", "acq_default.npz"))

        class FakeAcq(object):
            """Stands in for the GPU search of this rank's PRNs (no GPU here): returns the golden rows."""

            def __init__(self):
                self.settings = type("S", (), {"acqSatelliteList": range(1, 33)})()
                self.internals = None
                self.results = None

            def acquire(self, sig, n_blocks=2, noncoh=False, prn_indices=None):
                self.seen = list(prn_indices)
                self.carrFreq = g["carrFreq"].copy()
                self.codePhase = g["codePhase"].copy()
                self.peakMetric = g["peakMetric"].copy()
                self.internals = dict(freqBin=g["freqBin"].copy(), fineIdx=g["fineIdx"].copy())

        acq = FakeAcq()
        sh.acquire_sharded(acq, None, rank, world, sh.HostGather(dist))
        ok = (np.array_equal(acq.results.carrFreq, g["carrFreq"]) and
              np.array_equal(acq.results.codePhase, g["codePhase"]) and
              np.array_equal(acq.results.peakMetric, g["peakMetric"]) and
              acq.seen == list(sh.plan_shards(32, world)[rank]))
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def test_peak_gather_world_size_2_gloo():
    # torch is imported in the spawned ranks only: torch loads its own copies of the HIP and HSA runtimes, and a test
    # process that has libsgx's runtime up on a GPU must not hold two of them
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    got = dict(q.get(timeout=10) for _ in range(2))
    assert got == {0: True, 1: True}


def test_bench_self_launch_refuses_without_enough_devices():
    """bench.py --gpus 2 with WORLD_SIZE unset starts its own ranks; on a box with fewer devices (here: none) it
    exits non-zero and prints no JSON line - it never degrades silently to a 1-GPU measurement."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    if pkg()._native.device_count() >= 2:
        pytest.skip("this box has two GPUs")
    assert r.returncode != 0
    assert b"n_gpus" not in r.stdout
    assert b"refusing" in r.stderr


def test_bench_launcher_starts_one_child_per_rank(tmp_path, monkeypatch):
    """launch_ranks: N children with RANK/LOCAL_RANK/WORLD_SIZE/SGX_DEVICE/MASTER_* set, rank 0's stdout relayed,
    a failing rank makes the launcher fail."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    stub = tmp_path / "rank.py"
    stub.write_text("import os, sys\n"
                    "r = int(os.environ['RANK']); w = int(os.environ['WORLD_SIZE'])\n"
                    "assert os.environ['SGX_DEVICE'] == os.environ['LOCAL_RANK'] == str(r)\n"
                    "assert os.environ['MASTER_ADDR'] == '127.0.0.1' and int(os.environ['MASTER_PORT']) > 0\n"
                    "open(os.path.join(%r, 'seen%%d' %% r), 'w').write(str(w))\n"
                    "print('{\"n_gpus\": %%d}' %% w) if r == 0 else None\n"
                    "sys.exit(int(os.environ.get('FAIL_RANK', '-1')) == r)\n" % str(tmp_path))
    monkeypatch.setattr(bench, "count_devices_in_child", lambda: 4)
    monkeypatch.setattr(bench, "__file__", str(stub))
    monkeypatch.setattr(bench.os.path, "abspath", lambda p: p)
    assert bench.launch_ranks(3, []) == 0
    assert sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("seen")) == ["seen0", "seen1", "seen2"]
    monkeypatch.setenv("FAIL_RANK", "2")
    assert bench.launch_ranks(3, []) == 1
    assert bench.launch_ranks(5, []) == 3   # more ranks than devices


def _rdv_worker(rank, world, key, q):
    sys.path.insert(0, ROOT)
    rv = importlib.import_module("softgnss-python_amd.rendezvous")
    g = rv.HostGroup(rank, world, key=key, timeout=60)
    try:
        got = g.gather({"rank": rank, "blob": bytes([rank]) * 1000})
        g.barrier()
        q.put((rank, [x["rank"] for x in got], g.max(10.0 + rank), g.broadcast("id" if rank == 0 else None),
               all(x["blob"] == bytes([x["rank"]]) * 1000 for x in got)))
    finally:
        g.close()


def test_socket_rendezvous_world_size_3():
    """softgnss-python_amd/rendezvous.py: what bench.py uses between the ranks instead of torch.distributed."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    key = "t%d" % os.getpid()
    procs = [ctx.Process(target=_rdv_worker, args=(r, 3, key, q)) for r in range(3)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    got = sorted(q.get(timeout=10) for _ in range(3))
    assert [g[0] for g in got] == [0, 1, 2]
    for g in got:
        assert g[1] == [0, 1, 2] and g[2] == 12.0 and g[3] == "id" and g[4]


def _stub_env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["SGX_BENCH_PKG"] = "bench_stub"
    env["PYTHONPATH"] = os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
    return env


def _rdv_rank0(key, q):
    import importlib
    rv = importlib.import_module("softgnss-python_amd.rendezvous")
    os.environ["SGX_RDV_TOKEN"] = "sesame"
    g = rv.HostGroup(0, 2, key=key, timeout=60)
    q.put(g.gather({"r": 0, "blob": b"\x00\xff"}))
    g.close()


def test_socket_rendezvous_admits_only_its_own_ranks():
    """Rank 0 listens in the abstract AF_UNIX name space, which has no file permissions: a connection that sends
    something that is not the hello (a pickle, say), one without the launcher's token, one that claims a rank outside
    1 .. world-1 are all dropped; the real rank 1 then completes the group.  Nothing is ever unpickled."""
    import importlib
    import json
    import multiprocessing as mp
    import pickle
    import socket
    import struct
    import time
    rv = importlib.import_module("softgnss-python_amd.rendezvous")
    key = "t%d" % os.getpid()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p0 = ctx.Process(target=_rdv_rank0, args=(key, q))
    p0.start()
    addr = "\0sgx-rendezvous-%s-%s" % (key, os.environ.get("TORCHELASTIC_RUN_ID", "x"))

    def rogue(payload):
        deadline = time.time() + 60
        while True:
            c = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
            try:
                c.connect(addr)
                break
            except (ConnectionRefusedError, FileNotFoundError):
                c.close()
                assert time.time() < deadline
                time.sleep(0.05)
        c.sendall(struct.pack("<Q", len(payload)) + payload)
        c.settimeout(10)
        try:
            assert c.recv(1) == b""          # dropped: the server closes the connection
        except (ConnectionError, socket.timeout):
            pass
        c.close()

    class Boom(object):
        def __reduce__(self):
            return (os.system, ("touch /tmp/sgx_rdv_pwned_%d" % os.getpid(),))

    rogue(pickle.dumps(Boom()))
    rogue(json.dumps({"rank": 1, "token": "guess"}).encode())
    rogue(json.dumps({"rank": 7, "token": "sesame"}).encode())
    assert not os.path.exists("/tmp/sgx_rdv_pwned_%d" % os.getpid())
    os.environ["SGX_RDV_TOKEN"] = "sesame"
    try:
        g = rv.HostGroup(1, 2, key=key, timeout=60)
        got = g.gather({"r": 1, "blob": b"abc"})
        g.close()
    finally:
        os.environ.pop("SGX_RDV_TOKEN", None)
    assert got == [{"r": 0, "blob": b"\x00\xff"}, {"r": 1, "blob": b"abc"}] and q.get(timeout=60) == got
    p0.join(60)
    assert p0.exitcode == 0


def test_bench_two_ranks_end_to_end_against_a_stand_in_package():
    """`bench.py --gpus 2` from the self-launch to the JSON line, with tests/bench_stub.py answering for the GPU
    package: two ranks rendezvous, search 16 PRNs each, the RCCL transport is refused (the stand-in has none) so
    both fall back to the host gather AND SAY SO, rank 0 reports the max over ranks, per-rank extremes and the
    config-4 leg; PyTorch is never imported."""
    import json
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--ms", "50", "--no-cpu-baseline", "--full"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=_stub_env(), timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["config"]["prns_per_gpu"] == 16 and d["config"]["peak_gather"] == "host-socket"
    assert d["per_rank_peak_gather"] == ["host-socket"] and set(d["per_rank"]) == {"step_ms", "track_kernel_ms", "acquire_ms"}
    assert d["per_rank"]["step_ms"]["max"] >= d["per_rank"]["step_ms"]["min"] > 0
    assert abs(d["ms_per_step"] - d["per_rank"]["step_ms"]["max"]) < 1e-9          # the max over ranks is the figure
    assert d["acq_config4"]["sharded_result_equals_single_gpu"] is True
    assert d["value"] == pytest.approx(2 * d["config"]["record_samples"] / (d["ms_per_step"] * 1e-3) / 1e6)
    assert b"using host gather" in r.stderr
    # the same command under an external launcher's environment (one process, WORLD_SIZE=1) still prints its line
    code = "import sys; sys.argv=['bench.py','--steps','1','--warmup','0','--ms','50','--no-cpu-baseline']; import runpy; " \
           "runpy.run_path(%r, run_name='__main__'); assert 'torch' not in sys.modules" % os.path.join(ROOT, "bench.py")
    r1 = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=_stub_env(),
                        timeout=300)
    assert r1.returncode == 0, r1.stderr.decode()
    assert json.loads([ln for ln in r1.stdout.decode().splitlines() if ln.startswith("{")][0])["n_gpus"] == 1


def test_bench_plain_run_times_the_step_only_and_dumps_its_outputs(tmp_path):
    """A plain `bench.py` (no --full) with tests/bench_stub.py answering for the GPU package: the JSON line holds the
    headline figures and none of the side measurements, --steps sets the timed steps, and --dump-outputs writes the
    last step's search results, channel table and tracking series as float64 .npy files, the same on every run.  A
    series larger than the limit is written as a fixed sample of its milliseconds."""
    import importlib.util
    import json
    import subprocess
    import types
    dumps = []
    for k in range(2):
        d = tmp_path / ("out%d" % k)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--ms", "50",
                            "--dump-outputs", str(d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=_stub_env(),
                           timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["n_gpus"] == 1 and line["ms_per_step"] > 0
        assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["value"] == pytest.approx(line["config"]["record_samples"] / (line["ms_per_step"] * 1e-3) / 1e6)
        assert not set(line) & {"roofline", "acq_config4", "roofline_acq", "roofline_many_channels", "from_file",
                                "concurrent_records", "cpu_baseline", "float_records", "many_channels_other_types"}
        dumps.append({f.name: np.load(str(f)) for f in d.iterdir()})
    got = dumps[0]
    assert sum(a.nbytes for a in got.values()) <= 64 * 10 ** 6
    assert all(f.endswith(".npy") for f in got) and all(a.dtype == np.float64 for a in got.values())
    assert got["acq_codePhase.npy"].shape == (32,) and got["channels_PRN.npy"].shape == (8,)
    assert got["trk_absoluteSample.npy"].shape == (int(np.sum(got["channels_PRN.npy"] != 0)), 50)
    assert len([f for f in got if f.startswith("trk_")]) == 13
    assert set(dumps[1]) == set(got) and all(np.array_equal(dumps[1][f], got[f]) for f in got)
    # the limit: a seeded sample of the milliseconds, the same every time, its indices written beside it
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    acq = types.SimpleNamespace(results=np.rec.fromarrays([np.arange(32.0)] * 3, names="carrFreq,codePhase,peakMetric"),
                                channels=np.rec.fromarrays([np.arange(1, 9), np.ones(8), np.zeros(8)],
                                                           names="PRN,acquiredFreq,codePhase"))
    series = np.arange(8 * 3 * 1000, dtype=np.float64).reshape(8, 3, 1000)
    for k in range(2):
        bench.dump_outputs(str(tmp_path / ("small%d" % k)), acq, series, ("a", "b", "c"), limit=64 * 1024)
    a, b = (np.load(str(tmp_path / ("small%d" % k) / "trk_b.npy")) for k in range(2))
    idx = np.load(str(tmp_path / "small0" / "trk_ms_index.npy"))
    total = sum(os.path.getsize(str(f)) for f in (tmp_path / "small0").iterdir())
    assert 0 < a.shape[1] == idx.size < 1000 and np.array_equal(a, b) and np.array_equal(a, series[:, 1, idx.astype(int)])
    assert total <= 64 * 1024 + 128 * len(list((tmp_path / "small0").iterdir()))   # (.npy headers on top)


def test_bench_launcher_stops_the_other_ranks_when_one_dies():
    """A rank that exits early (no device, RCCL failure) must not leave the others waiting at a barrier: the launcher
    sees the first non-zero exit, stops the rest and returns non-zero - quickly, and without a JSON line."""
    import subprocess
    import time
    env = _stub_env()
    env["SGX_STUB_FAIL_RANK"] = "1"
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--ms", "50", "--no-cpu-baseline"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                       timeout=300)
    assert r.returncode != 0 and b"n_gpus" not in r.stdout
    assert b"ranks failed" in r.stderr and time.time() - t0 < 60
