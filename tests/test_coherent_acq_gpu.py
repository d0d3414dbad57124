"""Coherent multi-millisecond acquisition on the GPU (sgx_acquire_coherent, csrc/sgx_acq.hip): the 1-ms case against
sgx_acquire bit for bit, small searches against the numpy contract (tests/coherent_acq_spec.py) on both paths and both
input types, a weak-signal scene the reference's search cannot see, that scene tracked to the end, and the error paths.
Run with -m gpu."""
import numpy as np
import pytest

import coherent_acq_spec as spec
import weak_scene
from conftest import pkg

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


WEAK_MS = 1100


@pytest.fixture(scope="module")
def weak(m):
    host = weak_scene.generate(WEAK_MS)
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


def test_weak_scene_needs_coherent_windows(m, weak):
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
