"""Strong-signal cancellation on the GPU (sgx_if_cancel, csrc/sgx_cancel.hip; TrackingResult.cancel;
Settings.strongSignalCancellation): the kernel against the numpy contract (tests/cancel_spec.py) and against the host twin on
every case of tests/cancel_cases.py under the rule of cancel_cases.compare - equal bytes wherever v lies farther than 1e-6
from a half-integer, clip counts exact -, and the near-far scene of tests/nearfar_scene.py through the Python layer with the
GPU's own search and tracking - on a DeviceFile at offset 0 and at an offset that is no multiple of 16, through
postProcessing() on a file at skipNumberOfBytes 0 and 5000 (the window of the file that Settings._cancel_strong uploads) and
behind a record stage (the resident path: positions are samples of the prepared record).  Run with -m gpu."""
import subprocess
import sys

import numpy as np
import pytest

import cancel_cases as cases
import cancel_spec as spec
import nearfar_scene as nf
from conftest import ROOT, pkg
from test_gpu_parity import TRK_TOL, _trk_err

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", cases.NAMES)
def test_kernel_equals_the_contract_and_the_host_twin(name, capsys):
    m = pkg()
    n = m._native
    c = cases.get(name)
    ctx = m.engine.get_context(c["s"], 0)
    rec = ctx.upload(c["x"])
    try:
        kw = dict(ms_done=c["ms_done"], rec_file_offset=c["off"])
        out = ctx.if_cancel(rec, c["chans"], c["series"], c["amp"], **kw)
        y, clipped, kernel_ms = out.download(), out.clipped, ctx.cancel_timing()
        out.free()
        again = ctx.if_cancel(rec, c["chans"], c["series"], c["amp"], **kw)
        y2, clipped2 = again.download(), again.clipped
        again.free()
        assert np.array_equal(rec.download(), c["x"])            # the input record is not written
    finally:
        rec.free()
    excluded = cases.compare(name, y, clipped)
    assert y.tobytes() == y2.tobytes() and clipped == clipped2   # two calls: the same bytes
    yh, ch = n.cancel_host(c["s"], c["x"], c["chans"], c["series"], c["amp"], **kw)
    want, v, _, covered = cases.expected(name)
    differ = np.flatnonzero(y != yh)
    assert np.all(spec.decisions(v, covered)[differ]) and clipped == ch, (name, differ[:8])
    assert kernel_ms > 0
    with capsys.disabled():
        print("\n[cancel] %s: %d samples, %d excluded, %d differ from the host twin, %d clipped, kernel %.3f ms"
              % (name, y.size, excluded, differ.size, clipped, kernel_ms))


def test_refusals_on_the_device_launch_nothing():
    m = pkg()
    n = m._native
    c = cases.get("rate2")
    ctx = m.engine.get_context(c["s"], 0)
    rec = ctx.upload(c["x"])
    try:
        for kw in (dict(data_type=n.DT_UINT8), dict(data_type=n.DT_INT16), dict(ms_done=[12, 13, 12]),
                   dict(rec_file_offset=int(min(ch[2] for ch in c["chans"])) + 1)):
            with pytest.raises(n.SgxError) as e:
                ctx.if_cancel(rec, c["chans"], c["series"], c["amp"], **kw)
            assert e.value.code == (n.SGX_E_RANGE if "rec_file_offset" in kw else n.SGX_E_ARG)
        bad = np.array(c["amp"])
        bad[1, 3, 0] = np.inf
        with pytest.raises(n.SgxError) as e:
            ctx.if_cancel(rec, c["chans"], c["series"], bad)
        assert e.value.code == n.SGX_E_ARG and "channel 1 block 3" in str(e.value)
        many = [c["chans"][0]] * 33
        with pytest.raises(n.SgxError) as e:
            ctx.if_cancel(rec, many, np.repeat(c["series"][:1], 33, axis=0), np.repeat(c["amp"][:1], 33, axis=0))
        assert e.value.code == n.SGX_E_ARG
        short = ctx.upload(c["x"][:int(c["series"][:, 0, -1].max()) - 1])
        try:
            with pytest.raises(n.SgxError) as e:
                ctx.if_cancel(short, c["chans"], c["series"], c["amp"])
            assert e.value.code == n.SGX_E_RANGE
        finally:
            short.free()
        assert np.array_equal(rec.download(), c["x"])
    finally:
        rec.free()


@pytest.fixture(scope="module")
def scene_run():
    """The near-far record in HBM, searched over [2 n, 13 n) and its detections tracked for 40 ms, all on the GPU."""
    m = pkg()
    s = m.Settings()
    s.samplingFreq, s.IF, s.numberOfChannels, s.msToProcess = nf.FS, nf.IF, 4, float(nf.MS_TRACKED)
    ctx = m.engine.get_context(s, 0)
    rec = ctx.upload(nf.record())
    n = s.samplesPerCode
    a = m.AcquisitionResult(s, device=0)
    a.acquire(m.DeviceSignal(rec, 2 * n, 11 * n), prn_indices=[p - 1 for p in nf.SEARCHED])
    a.preRun()
    t = m.TrackingResult(a, device=0)
    t.track(m.DeviceFile(rec))
    yield m, s, ctx, rec, n, a, t
    rec.free()


def _detections(a):
    return [p for p in nf.SEARCHED if a.carrFreq[p - 1] > 0]


def test_near_far_scene_through_the_python_layer(scene_run, capsys):
    """The raw search detects PRN 1 and 3 only; TrackingResult.cancel of both; the search of the cleaned record detects PRN
    7 and 11 within one sample of code phases 4000 and 15000 and leaves PRN 14 and 19 below acqThreshold; PRN 7 is then
    tracked on the cleaned record for 40 ms; and the cleaned record equals the contract's on the GPU's own series."""
    m, s, ctx, rec, n, a, t = scene_run
    assert _detections(a) == [1, 3] and list(t.results.PRN) == [1, 3]
    cleaned = t.cancel(m.DeviceFile(rec))
    try:
        assert isinstance(cleaned, m.DeviceFile) and cleaned.file_offset == 0 and len(cleaned.record) == len(rec)
        assert cleaned.PRN == [1, 3] and cleaned.kernel_ms > 0
        chans = [(int(c.PRN), float(c.acquiredFreq), float(c.codePhase)) for c in a.channels if c.PRN != 0]
        so = nf.settings()
        amp = spec.design(t.series, spec.states(so, len(rec), 0, chans, t.series, None))
        want, v, clipped, covered = spec.cancel(so, nf.record(), 0, chans, t.series, None, amp)
        y = cleaned.record.download()
        differ = np.flatnonzero(y != want)
        assert np.all(spec.decisions(v, covered)[differ]) and differ.size <= 1e-4 * y.size and cleaned.clipped == clipped
        b = m.AcquisitionResult(s, device=0)
        b.acquire(m.DeviceSignal(cleaned.record, 2 * n, 11 * n), prn_indices=[p - 1 for p in nf.SEARCHED])
        found = _detections(b)
        with capsys.disabled():
            print("\n[cancel] GPU search, peakMetric of PRN %s: raw %s, cleaned %s" % (
                nf.SEARCHED, np.round([a.peakMetric[p - 1] for p in nf.SEARCHED], 2),
                np.round([b.peakMetric[p - 1] for p in nf.SEARCHED], 2)))
        assert 7 in found and 11 in found and 14 not in found and 19 not in found
        assert abs(b.codePhase[6] - 4000) <= 1 and abs(b.codePhase[10] - 15000) <= 1
        assert b.peakMetric[13] < s.acqThreshold and b.peakMetric[18] < s.acqThreshold
        # the same after .results was assigned from a cache
        t2 = m.TrackingResult(a, device=0)
        t2.results = t.results
        c2 = t2.cancel(m.DeviceFile(rec), rows=[0, 1])
        assert c2.record.download().tobytes() == y.tobytes()
        c2.record.free()
        one = t.cancel(m.DeviceFile(rec), rows=[1], smooth=5)                # PRN 3 alone, smoothed amplitudes
        assert one.PRN == [3] and np.any(one.record.download() != y)
        one.record.free()
        with pytest.raises(ValueError):
            t.cancel(m.DeviceFile(rec), rows=[2])
        # PRN 7 tracked on the cleaned record
        c7 = m.AcquisitionResult(s, device=0)
        c7.acquire(m.DeviceSignal(cleaned.record, 2 * n, 11 * n), prn_indices=[6])
        c7.preRun()
        t7 = m.TrackingResult(c7, device=0)
        t7.track(cleaned)
        assert t7.has_results() and t7.series.shape == (1, 13, nf.MS_TRACKED) and list(t7.results.PRN) == [7]
        env = np.sqrt(t7.series[0, [4, 3, 5]] ** 2 + t7.series[0, [6, 7, 8]] ** 2)[:, 20:].mean(axis=1)     # E P L
        assert env[1] > env[0] and env[1] > env[2], env
    finally:
        cleaned.record.free()


def test_command_line_cancel_strong(scene_run, tmp_path):
    """main.py --cancel-strong on the near-far record: PRN 1 and 3 are found and tracked, cancelled, PRN 7 and 11 found on
    the cleaned record and tracked in the two free channels: four satellites in the last quality table.  (The threshold is
    40 dB-Hz: over the first 40 ms the loops are still pulling in and the estimator reads 43 and 48 dB-Hz for the two.)"""
    path = str(tmp_path / "nearfar.bin")
    nf.record().tofile(path)
    r = subprocess.run([sys.executable, "-m", "softgnss-python_amd.main", path, "--fs", str(nf.FS), "--IF", str(nf.IF), "--ms",
                        str(nf.MS_TRACKED), "--channels", "4", "--no-probe", "--lock-detector", "--cancel-strong=40"],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "Cancelling PRN 1, 3" in r.stdout and "Found on the cleaned record: PRN 7, 11" in r.stdout, r.stdout[-3000:]
    tail = r.stdout[r.stdout.index("Found on the cleaned record"):]
    rows = [ln.split("|") for ln in tail.splitlines() if ln.startswith("|") and ln.count("|") == 6 and "PRN" not in ln]
    assert sorted(int(x[2]) for x in rows) == [1, 3, 7, 11], tail[-3000:]


def test_cancel_on_a_device_file_at_an_odd_offset(scene_run):
    """The record from byte 1003 of the file on (no multiple of 16, in front of the first code start) as
    DeviceFile(window, 1003): searched over the same bytes [2 n, 13 n) of the file, tracked, cancelled.  The cleaned record
    keeps the offset and equals the contract at that offset on the GPU's own series, as the scene test's does at offset 0."""
    m, s, ctx, _, n, _, _ = scene_run
    off = 1003
    assert off % 16 != 0 and off < min(nf.CODE_STARTS)
    host = nf.record()[off:]
    rec = ctx.upload(host)
    cleaned = None
    try:
        a = m.AcquisitionResult(s, device=0)
        a.acquire(m.DeviceSignal(rec, 2 * n - off, 11 * n), prn_indices=[p - 1 for p in nf.SEARCHED])
        a.preRun()
        assert _detections(a) == [1, 3]
        t = m.TrackingResult(a, device=0)
        t.track(m.DeviceFile(rec, off))
        assert list(t.results.PRN) == [1, 3] and t.series.shape == (2, 13, nf.MS_TRACKED)
        cleaned = t.cancel(m.DeviceFile(rec, off))
        assert cleaned.file_offset == off and len(cleaned.record) == len(rec) and cleaned.PRN == [1, 3]
        chans = [(int(c.PRN), float(c.acquiredFreq), float(c.codePhase)) for c in a.channels if c.PRN != 0]
        assert all(abs(c[2] - want) <= 1 for c, want in zip(chans, nf.CODE_STARTS))           # positions of the FILE
        so = nf.settings()
        amp = spec.design(t.series, spec.states(so, len(host), off, chans, t.series, None))
        want, v, clipped, covered = spec.cancel(so, host, off, chans, t.series, None, amp)
        y = cleaned.record.download()
        differ = np.flatnonzero(y != want)
        assert np.all(spec.decisions(v, covered)[differ]) and differ.size <= 1e-4 * y.size and cleaned.clipped == clipped
        assert np.any(y != host) and np.array_equal(rec.download(), host)
    finally:
        if cleaned is not None:
            cleaned.record.free()
        rec.free()


def _post_processing(m, path, **more):
    """postProcessing() of a file with the settings of test_command_line_cancel_strong.  Returns (settings, acquisition
    results, tracking results)."""
    s = m.Settings()
    s.fileName, s.samplingFreq, s.IF, s.msToProcess, s.numberOfChannels = path, nf.FS, nf.IF, float(nf.MS_TRACKED), 4
    s.lockDetector, s.strongSignalCancellation, s.cancelCNoThreshold = True, True, 40.0
    for k, val in more.items():
        assert hasattr(s, k), k
        setattr(s, k, val)
    acq, trk, _ = s.postProcessing()
    return s, acq, trk


def test_post_processing_at_a_file_offset_equals_the_run_at_offset_zero(tmp_path, capsys):
    """The near-far record behind 5000 arbitrary bytes, skipNumberOfBytes = 5000: Settings._cancel_strong uploads the
    file from byte 4096 on and searches the cleaned record 904 + n samples into it.  Measured against the run on the plain
    file: the same four satellites joined, the same acquisition results, absoluteSample 5000 further on, and the six
    correlator series within the bar of tests/test_gpu_parity.py."""
    m = pkg()
    K = 5000
    plain, padded = str(tmp_path / "nearfar.bin"), str(tmp_path / "padded.bin")
    nf.record().tofile(plain)
    with open(padded, "wb") as fh:
        fh.write(np.random.default_rng(5).integers(-128, 128, K).astype(np.int8).tobytes())
        fh.write(nf.record().tobytes())
    s0, a0, t0 = _post_processing(m, plain)
    s1, a1, t1 = _post_processing(m, padded, skipNumberOfBytes=K)
    assert K // 4096 * 4096 == 4096 and K - 4096 == 904
    for a, t in ((a0, t0), (a1, t1)):
        assert sorted(int(p) for p in t.results.PRN) == [1, 3, 7, 11] and list(t.results.PRN[:2]) == [1, 3]
        assert [int(p) + 1 for p in np.flatnonzero(np.asarray(a.results["carrFreq"]) > 0)] == [1, 3, 7, 11]
    assert list(t1.results.PRN) == list(t0.results.PRN)
    for k in ("codePhase", "carrFreq"):
        assert np.array_equal(np.asarray(a1.results[k]), np.asarray(a0.results[k])), k
    assert t0.series.shape == t1.series.shape == (4, 13, nf.MS_TRACKED)
    assert np.array_equal(t1.series[:, 0] - K, t0.series[:, 0])
    err = _trk_err(t1.series, t0.series)
    with capsys.disabled():
        print("\n[cancel] postProcessing at skipNumberOfBytes %d against 0: correlator series %.3g of RMS|P| (bar %.0e)"
              % (K, err, TRK_TOL))
    assert err < TRK_TOL


def test_post_processing_behind_a_record_stage(tmp_path):
    """The resident path: the scene's file with a DC offset through the conditioning stage (byte-exact against its contract,
    tests/test_cond_gpu.py), strongSignalCancellation on.  _resident_processing hands Settings._cancel_strong a DeviceFile of
    the PREPARED record.  What tests/test_cancel_host.py shows with the oracle on that record holds on the device: PRN 1 and
    3 tracked and cancelled, PRN 7 and 11 found and tracked on the cleaned record, their code phases within one sample of
    the oracle's."""
    m = pkg()
    path = str(tmp_path / "offset.bin")
    nf.offset_file().tofile(path)
    s, acq, trk = _post_processing(m, path, frontEndConditioning=True, **nf.COND)
    raw, chans, series, clean = nf.oracle_run_prepared()
    joined = [int(p) for p in trk.results.PRN]
    assert joined[:2] == [1, 3] and sorted(joined) == [1, 3, 7, 11], joined
    assert trk.series.shape == (4, 13, nf.MS_TRACKED) and s.lastConditioning["samples"] == nf.prepared_record().size
    for p in nf.WEAK:
        assert abs(float(acq.results["codePhase"][p - 1]) - clean[p][1]) <= 1, (p, acq.results["codePhase"][p - 1], clean[p][1])
