"""Coherent multi-millisecond acquisition on the GPU (sgx_acquire_coherent, csrc/sgx_acq.hip): the 1-ms case against
sgx_acquire bit for bit, small searches against the numpy contract (tests/coherent_acq_spec.py) on both paths and both
input types, dense scenes with a satellite on every class of bin, phi row, run and batch (tests/dense_scene.py; conditioned
on the CPU by tests/test_coherent_acq_cases.py), the reference's IndexError, a weak-signal scene the reference's search
cannot see, that scene tracked to the end, and the error paths.  Run with -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

import coherent_acq_spec as spec
import dense_child
import dense_scene
import weak_scene
from conftest import pkg
from oracle import softgnss_oracle as orc

pytestmark = pytest.mark.gpu

N = 38192
KEYS = ("carrFreq", "codePhase", "peakMetric", "freqBin", "fineIdx")


@pytest.fixture(scope="module")
def m():
    return pkg()


def test_one_ms_is_sgx_acquire_bit_for_bit(m, default_record):
    s = m.Settings()
    ctx = m.engine.get_context(s, 0)
    rec = ctx.upload(default_record[:11 * N])
    try:
        for blocks, noncoh in ((2, False), (10, True)):
            want = ctx.acquire(rec, 0, 11 * N, list(range(32)), n_blocks=blocks, noncoh=noncoh)
            got = ctx.acquire_coherent(rec, 0, 11 * N, list(range(32)), coherent_ms=1, n_windows=blocks, noncoh=noncoh,
                                       bin_step_hz=500.0)
            assert np.sum(want["carrFreq"] > 0) >= 4
            for k in KEYS:
                assert np.array_equal(got[k], want[k]), (blocks, k)
    finally:
        rec.free()


STRONG = ((1, 45.0, 210.0, 5000), (6, 44.0, -380.0, 20000))


@pytest.fixture(scope="module")
def strong_record():
    return weak_scene.generate(42, sats=STRONG, seed=11)


@pytest.mark.parametrize("T,M,noncoh,step,f64,band,path,runs", [
    (2, 2, False, None, False, 1.0, "shift", False),
    (4, 3, True, None, False, 1.0, "shift", False),
    (10, 2, False, None, True, 1.0, "shift", False),
    (10, 2, True, None, False, 1.0, "shift", False),
    (2, 20, False, None, False, 5.0, "shift", True),    # 21 bins x 20 windows = 420 rows per PRN: runs of 16 + 4 windows
    (2, 20, True, None, True, 5.0, "shift", True),      # ... runs of 17 + 4 bins
    (10, 2, False, None, False, 14.0, "shift", True),   # the default band: 281 bins x 2 windows, one window per run
    (2, 2, False, 15.0, False, 1.0, "direct", False),
    (4, 2, True, 11.0, True, 1.0, "direct", False),
])
def test_small_searches_match_the_contract(m, strong_record, T, M, noncoh, step, f64, band, path, runs):
    s = m.Settings()
    s.acqSearchBand = band
    g = spec.grid(s, T, M, noncoh, step)
    assert g["path"] == path
    plan = m._native.acquire_coherent_plan(s, T, M, noncoh, step)
    assert (plan["bin_runs"], plan["prn_chunk"]) == (g["bin_runs"], g["prn_chunk"])
    assert (plan["bin_runs"] > 1) == runs, plan
    n = (max(11, T * M) + 1) * N
    x = strong_record[:n]
    prns = [1, 6, 9]
    ctx = m.engine.get_context(s, 0)
    if f64:
        got = ctx.acquire_coherent_f64(x.astype(np.float64), prns, coherent_ms=T, n_windows=M, noncoh=noncoh,
                                       bin_step_hz=step)
    else:
        rec = ctx.upload(x)
        try:
            got = ctx.acquire_coherent(rec, 0, n, prns, coherent_ms=T, n_windows=M, noncoh=noncoh, bin_step_hz=step)
        finally:
            rec.free()
    want = spec.acquire(s, x, T, M, noncoh, step, prn_indices=prns)
    assert want["carrFreq"][1] > 0 and want["carrFreq"][6] > 0
    for k in ("carrFreq", "codePhase", "freqBin", "fineIdx"):
        assert np.array_equal(np.asarray(got[k]), want[k][prns]), (k, got[k], want[k][prns])
    assert np.allclose(got["peakMetric"], want["peakMetric"][prns], rtol=1e-9, atol=0)


def _dense_compare(c, got, want):
    """Exact indices and peakMetric to 1e-9 for every searched PRN (all of them placed); PRNs of the case's literal drop
    list keep peakMetric only, single-window satellites of its no_fine list keep all but the fine index."""
    prns = np.asarray(c.prns)
    assert np.allclose(got["peakMetric"], want["peakMetric"][prns], rtol=1e-9, atol=0), \
        (got["peakMetric"], want["peakMetric"][prns])
    keep = np.array([p not in c.drop for p in c.prns])
    fine = keep & np.array([p not in c.no_fine for p in c.prns])
    assert keep.sum() >= len(c.prns) - 2
    assert np.all(want["carrFreq"][prns] > 0)
    for k, sel in (("codePhase", keep), ("freqBin", keep), ("fineIdx", fine), ("carrFreq", fine)):
        assert np.array_equal(np.asarray(got[k])[sel], want[k][prns][sel]), (k, got[k], want[k][prns])


def _dense_plan(m, c):
    s = m.Settings()
    s.samplingFreq, s.IF, s.acqSearchBand = c.s.samplingFreq, c.s.IF, c.s.acqSearchBand
    plan = m._native.acquire_coherent_plan(s, c.T, c.M, c.noncoh, c.step)
    for k in ("n_bins", "n_phi", "path", "prn_chunk", "bin_runs"):
        assert plan[k] == c.g[k], (k, plan, c.g[k])
    assert (plan["path"], plan["prn_chunk"], plan["bin_runs"]) == (c.path, c.prn_chunk, c.bin_runs)


@pytest.mark.parametrize("name", [c.name for c in dense_scene.CASES])
def test_dense_scenes_match_the_contract(m, name):
    """One satellite per searched PRN on chosen bins (edge bins, every phi row, both sides of each cut between runs, single
    windows on both sides of a cut between runs of windows), so that a wrong shift, row offset or batch offset anywhere
    moves an asserted index.  The contract runs over PRNs in child processes that never open the GPU."""
    c = dense_scene.BY_NAME[name]
    _dense_plan(m, c)
    want = c.reference()
    got = dense_child.run_case(m, c)
    _dense_compare(c, got, want)


def test_dense_scene_with_the_unfused_fine_search(m, tmp_path):
    """SGX_ACQ_FINE_V1=1 (the fine search as separate kernels, here with per-detection ranges at N = 38 192) is read from
    the environment, so the search runs in a fresh child process; this process's environment stays as it is."""
    c = dense_scene.BY_NAME["2x2_offset"]
    want = c.reference()
    out = str(tmp_path / "fine_v1.npz")
    env = dict(os.environ, SGX_ACQ_FINE_V1="1")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dense_child.py")
    r = subprocess.run([sys.executable, child, c.name, out], env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    _dense_compare(c, dict(np.load(out)), want)


@pytest.mark.parametrize("direct", [False, True])
def test_index_error_of_the_reference(m, direct):
    """A peak at code phase spc exactly: the reference's exclusion list reaches index N (acquisition.py:152-162), the
    contract raises IndexError and the library returns SGX_E_INDEX with the reference's message, on both paths.  A peak at
    any other phase <= spc (sample 10 + 1 here) gives a list inside the row: no error from either, and equal results."""
    o, kw, p = dense_scene.index_error_case(direct)
    N = o.samplesPerCode
    spc = int(round(o.samplingFreq / o.codeFreqBasis))
    s = m.Settings()
    s.samplingFreq, s.IF, s.acqSearchBand = o.samplingFreq, o.IF, o.acqSearchBand
    assert m._native.acquire_coherent_plan(s, 2, 2, False, None)["path"] == ("direct" if direct else "shift")
    ctx = m.engine.get_context(s, 0)
    x = dense_scene.index_error_record(o)
    with pytest.raises(IndexError):
        np.zeros(N)[orc.exclusion_index(spc, N, spc)]
    with pytest.raises(IndexError):
        spec.acquire(o, x, 2, 2, False, None, prn_indices=[p])
    rec = ctx.upload(x)
    try:
        with pytest.raises(IndexError) as e:
            ctx.acquire_coherent(rec, 0, x.size, [p], **kw)
        assert m._native.SGX_E_INDEX == -4
        assert "IndexError: index %d is out of bounds for axis 1 with size %d" % (N, N) in str(e.value)
        assert "codePhase %d" % spc in str(e.value)
        with pytest.raises(IndexError):
            ctx.acquire_coherent_f64(x.astype(np.float64), [p], **kw)
    finally:
        rec.free()
    y = dense_scene.index_error_record(o, control=True)
    want = spec.acquire(o, y, 2, 2, False, None, prn_indices=[p])
    rec = ctx.upload(y)
    try:
        got = ctx.acquire_coherent(rec, 0, y.size, [p], **kw)
    finally:
        rec.free()
    assert want["codePhase"][p] == 11 and want["carrFreq"][p] > 0
    for k in ("carrFreq", "codePhase", "freqBin", "fineIdx"):
        assert got[k][0] == want[k][p], (k, got[k], want[k][p])
    assert np.allclose(got["peakMetric"][0], want["peakMetric"][p], rtol=1e-9, atol=0)


WEAK_MS = 1100


@pytest.fixture(scope="module")
def weak_host():
    return weak_scene.generate(WEAK_MS)


@pytest.fixture(scope="module")
def weak(m, weak_host):
    host = weak_host
    s = m.Settings()
    s.msToProcess = 1000.0
    ctx = m.engine.get_context(s, 0)
    rec = ctx.upload(host)
    yield s, rec
    rec.free()


def _truth_ok(s, a, p, dop, s0, T, M, step):
    npts = 1 << 22
    cph = a.codePhase[p]
    d = weak_scene.code_drift_samples(dop, T * M)
    assert s0 + min(0.0, d) - 2 <= cph <= s0 + max(0.0, d) + 2, (p, cph, s0, d)
    truth = s.IF + dop
    fbin = a.internals["freqBin"][p]
    assert abs(s.IF - s.acqSearchBand / 2 * 1000 + step * fbin - truth) <= step, (p, fbin)
    peak_f = (a.internals["fineIdx"][p] + 4) * s.samplingFreq / npts   # (carrFreq keeps the reference's slice index)
    assert abs(peak_f - truth) <= step, (p, peak_f, truth)


def _numpy_search_near_truth(s, x, p, dop, T, M, step):
    """The contract's non-coherent search of PRN index p over the 5 bins around the truth, and its fine search there:
    (freqBin, codePhase, fineIdx, smallest relative gap of the three arg-maxes)."""
    g = spec.grid(s, T, M, True, step)
    k0 = int(round((s.IF + dop - g["f0"]) / step))
    bins = list(range(k0 - 2, k0 + 3))
    sub = dict(g, freqs=g["freqs"][bins], n_bins=len(bins))
    spectra = np.fft.fft(spec.fold(s, x.astype(np.float64), sub), axis=-1)
    res, _ = spec.coarse(s, spectra, sub, np.fft.fft(orc.make_ca_table(s)[p]).conj())
    fbi = bins[int(res.max(1).argmax())]
    c = int(res.max(0).argmax())
    fine, _, top = spec.fine_search(s, g, x - x.mean(), p, c, fbi)
    gap = min(spec.rel_gap(spec._top2(res.max(1))), spec.rel_gap(spec._top2(res.max(0))), spec.rel_gap(top))
    return fbi, c, fine, gap


def test_weak_scene_needs_coherent_windows(m, weak, weak_host):
    s, rec = weak
    present = [p for p, _, _, _ in weak_scene.WEAK_SATS]
    ref = m.AcquisitionResult(s, device=0)
    ref.acquire(m.DeviceSignal(rec, 0, 11 * N))
    assert int(np.sum(ref.carrFreq[present] > 0)) <= len(present) // 2, ref.peakMetric[present]
    a = m.AcquisitionResult(s, device=0)
    a.acquire(m.DeviceSignal(rec, 0, 100 * N), n_blocks=10, noncoh=True, coherent_ms=10)
    assert np.all(a.carrFreq[present] > 0), a.peakMetric[present]
    absent = [p for p in range(32) if p not in present]
    assert np.all(a.carrFreq[absent] == 0) and np.all(a.peakMetric[absent] <= s.acqThreshold), a.peakMetric[absent]
    for p, _, dop, s0 in weak_scene.WEAK_SATS:
        _truth_ok(s, a, p, dop, s0, 10, 10, 50.0)
    # ... and exactly what the numpy contract finds in the 5 bins around each truth (the global peak lies there: _truth_ok).
    # A PRN whose numpy arg-maxes are within 1e-6 of a tie is not conclusive and keeps the bound above only.
    x = weak_host[:100 * N]
    for p, _, dop, s0 in weak_scene.WEAK_SATS:
        fbi, c, fine, gap = _numpy_search_near_truth(s, x, p, dop, 10, 10, 50.0)
        print("PRN index %d: numpy bin %d phase %d fine %d, gap %.2e" % (p, fbi, c, fine, gap))
        if gap < 1e-6:
            continue
        assert (a.internals["freqBin"][p], a.codePhase[p], a.internals["fineIdx"][p]) == (fbi, c, fine), p


def test_weak_scene_tracks_to_the_end(m, weak):
    s, rec = weak
    a = m.AcquisitionResult(s, device=0)
    a.acquire(m.DeviceSignal(rec, 0, 100 * N), n_blocks=10, noncoh=True, coherent_ms=10)
    a.preRun()
    t = m.TrackingResult(a, device=0)
    t.track(m.DeviceFile(rec))
    q = t.quality
    truth = {p + 1: cn0 for p, cn0, _, _ in weak_scene.WEAK_SATS}
    assert sorted(int(x) for x in q.PRN) == sorted(truth)
    for row in q:
        assert row.lostAtMs == -1, (row.PRN, row.lostAtMs)
        assert abs(row.medianCNo - truth[int(row.PRN)]) <= 3.0, (row.PRN, row.medianCNo)


def test_error_paths(m, weak):
    s, rec = weak
    ctx = m.engine.get_context(s, 0)
    nat = m._native
    with pytest.raises(nat.SgxError) as e:
        ctx.acquire_coherent(rec, 0, 50 * N, [0, 1], coherent_ms=10, n_windows=10, noncoh=True)
    assert e.value.code == nat.SGX_E_RANGE and "short" in str(e.value) and str(50 * N) in str(e.value)
    with pytest.raises(nat.SgxError) as e:
        ctx.acquire_coherent_f64(np.zeros(50 * N), [0, 1], coherent_ms=10, n_windows=10, noncoh=True)
    assert e.value.code == nat.SGX_E_RANGE and "short" in str(e.value)
    for kw in (dict(coherent_ms=21, n_windows=2), dict(coherent_ms=0, n_windows=2),
               dict(coherent_ms=10, n_windows=2, bin_step_hz=-1.0), dict(coherent_ms=10, n_windows=2, bin_step_hz=5.0)):
        with pytest.raises(nat.SgxError) as e:
            ctx.acquire_coherent(rec, 0, 100 * N, [0, 1], **kw)
        assert e.value.code == nat.SGX_E_ARG, kw
    with pytest.raises(ValueError):
        pkg("shard").acquire_sharded(m.AcquisitionResult(s, device=0), m.DeviceSignal(rec, 0, 100 * N), 0, 1, None,
                                     coherent_ms=10)
