"""C/N0 estimate and lock detector without a GPU: the numpy contract (tests/lock_spec.py) on synthetic prompts and on
counter sequences worked by hand, the new Settings attributes, the C struct, and TrackingResult's status logic against
a stand-in context.  The kernel against the contract is tests/test_track_quality_gpu.py (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

import lock_spec as spec
from conftest import pkg

T = 1e-3
W = 20


def _run(cno_dbhz, phase, seed, n_ms=4000):
    rng = np.random.default_rng(seed)
    i, q = spec.synthetic_prompts(rng, n_ms, cno_dbhz, phase)
    return spec.quality(i[None], q[None], T, 25.0, 0.85, W, 25)


@pytest.mark.parametrize("cno_dbhz", [35.0, 45.0, 60.0])
@pytest.mark.parametrize("phase", [0.0, 0.05])
def test_the_rotated_estimator_reads_the_true_cno(cno_dbhz, phase):
    cno, cl, ok, lost = _run(cno_dbhz, phase, seed=int(cno_dbhz * 10 + phase * 100))
    assert abs(np.median(cno) - cno_dbhz) < 0.6, np.median(cno)
    assert np.median(cl) >= 0.95
    assert lost[0] == -1


def test_a_static_phase_error_shows_in_the_carrier_lock_not_the_cno():
    cno, cl, ok, lost = _run(50.0, 0.3, seed=7)
    assert abs(np.median(cl) - np.cos(0.6)) < 0.01, np.median(cl)
    assert abs(np.median(cno) - 50.0) < 0.6
    assert lost[0] >= 0                                  # below the default 0.85: declared lost


def test_pure_noise_is_lost_within_50_windows():
    for seed in range(5):
        rng = np.random.default_rng(100 + seed)
        i, q = 100.0 * rng.standard_normal(4000), 100.0 * rng.standard_normal(4000)
        cno, cl, ok, lost = spec.quality(i[None], q[None], T, 25.0, 0.85, W, 25)
        assert 25 <= lost[0] < 50, lost


def test_counter_sequences_worked_by_hand():
    P, F = True, False
    assert spec.lock_scan([F] * 3, 3) == 2
    assert spec.lock_scan([F, F, P, F, F], 3) == 4              # 1 2 1 2 3
    assert spec.lock_scan([P, P, F, F, P, F, F], 3) == 6        # 0 0 1 2 1 2 3
    assert spec.lock_scan([F, P] * 20, 2) == -1                 # isolated fails recover: 1 0 1 0 ...
    assert spec.lock_scan([P] * 10 + [F, F, P, P, P, F, F], 3) == -1   # 1 2 1 0 0 1 2
    assert spec.lock_scan([F], 1) == 0
    assert spec.lock_scan([], 1) == -1


def test_windows_partial_windows_and_ms_done():
    rng = np.random.default_rng(3)
    i, q = spec.synthetic_prompts(rng, 2 * 105, 45.0, 0.0)
    i, q = i.reshape(2, 105), q.reshape(2, 105)
    cno, cl, ok, lost = spec.quality(i, q, T, 25.0, 0.85, 20, 2, ms_done=[105, 59])
    assert cno.shape == (2, 5)                                  # ms // W: the 5 ms tail is dropped
    assert np.all(np.isfinite(cno[0])) and np.all(np.isfinite(cno[1, :2]))
    assert np.all(np.isnan(cno[1, 2:])) and np.all(np.isnan(cl[1, 2:])) and not np.any(ok[1, 2:])
    R, X, P, A = spec.window_stats(i[0, 20:40], q[0, 20:40], 20)
    assert np.isclose(cno[0, 1], spec.cno_carr_lock(R, X, P, A, 20, T)[0][0], rtol=0, atol=1e-12)
    assert lost[1] == -1                                        # the windows past ms_done are not counted as fails
    cno, cl, ok, lost = spec.quality(i, q, T, 99.0, 0.85, 20, 2, ms_done=[105, 59])
    assert list(lost) == [1, 1]


def test_edge_values():
    z = np.zeros(4)
    cno, cl = spec.cno_carr_lock(*spec.window_stats(z, z, 4), 4, T)
    assert np.isnan(cno[0]) and np.isnan(cl[0])                 # P = 0; R = X = 0
    i = np.array([1.0, -1.0, 1.0, -1.0])                        # the rotated sum... of +-1 is 4: Psig = Ptot
    cno, cl = spec.cno_carr_lock(*spec.window_stats(i, z, 4), 4, T)
    assert cno[0] == np.inf and cl[0] == 1.0
    R, X, P, A = np.array([1.0]), np.array([0.0]), np.array([4.0]), np.array([0.0])
    assert spec.cno_carr_lock(R, X, P, A, 4, T)[0][0] == -np.inf


def test_settings_defaults():
    s = pkg().Settings()
    assert s.lockDetector is False
    assert s.cnoInterval == 20.0 and s.cnoThreshold == 25.0 and s.carrLockThreshold == 0.85 and s.maxLockFail == 25
    assert s.msToProcess == 37000.0 and s.pllNoiseBandwidth == 25.0      # the reference's attributes are unchanged


def test_lock_params_struct():
    n = pkg("_native")
    assert C.sizeof(n.LockParams) == 32
    p = n.lock_params(pkg().Settings())
    assert (p.window, p.max_fail, p.cno_min, p.carr_lock_min) == (20, 25, 25.0, 0.85)
    assert p.T == 1023 / 1023000.0


# ---- status logic against a stand-in context -------------------------------------------------------------------------

class FakeCtx(object):
    """track() and track_quality() of _native.Context, the latter answered by the numpy contract."""

    def __init__(self, lose=()):
        self.calls = []
        self.lose = set(lose)

    def track(self, rec, chans, ms, rec_file_offset=0, data_type=0):
        self.calls.append("track")
        rng = np.random.default_rng(11)
        out = np.zeros((len(chans), 13, ms))
        for c in range(len(chans)):
            out[c, 0] = 38192.0 * np.arange(1, ms + 1)
            if c in self.lose:
                out[c, 3], out[c, 7] = 100.0 * rng.standard_normal(ms), 100.0 * rng.standard_normal(ms)
            else:
                out[c, 3], out[c, 7] = spec.synthetic_prompts(rng, ms, 50.0, 0.0)
        return out, np.full(len(chans), ms, dtype=np.int32)

    def track_quality(self, i_p, q_p, params, ms_done=None):
        self.calls.append("quality")
        cno, cl, ok, lost = spec.quality(i_p, q_p, params.T, params.cno_min, params.carr_lock_min, params.window,
                                         params.max_fail, ms_done)
        return cno, cl, ok, lost.astype(np.int32)

    def timing(self):
        return dict(track_ms=1.0)


def _tracked(monkeypatch, lock, lose=(2, 5), ms=2000):
    m = pkg()
    ctx = FakeCtx(lose)
    monkeypatch.setattr(m.engine, "get_context", lambda s, d=None: ctx)
    s = m.Settings()
    s.numberOfChannels = 8
    s.msToProcess = float(ms)
    s.lockDetector = lock
    a = m.AcquisitionResult(s, device=0)
    prn = np.arange(1, 9)
    a._channels = np.rec.fromarrays([prn, np.full(8, 9548000.0), np.arange(8) * 100.0, ['T'] * 8],
                                    names='PRN,acquiredFreq,codePhase,status')
    t = m.TrackingResult(a, device=0)
    rec = type("Rec", (), {"__len__": lambda self: 10 ** 9})()
    t.track(m.DeviceFile(rec))
    return m, ctx, t


def test_lost_channels_get_status_dash(monkeypatch):
    m, ctx, t = _tracked(monkeypatch, True)
    assert ctx.calls == ["track", "quality"]
    assert [x.decode() if isinstance(x, bytes) else x for x in t.results.status] == \
        ['T', 'T', '-', 'T', 'T', '-', 'T', 'T']
    q = t.quality
    assert ctx.calls == ["track", "quality"]                    # computed once
    assert list(q.PRN) == list(range(1, 9))
    lost = q.lostAtMs
    assert np.all(lost[[2, 5]] > 0) and np.all(lost[[0, 1, 3, 4, 6, 7]] == -1)
    assert np.all(lost[[2, 5]] % 20 == 0) and np.all(lost[[2, 5]] <= 1000)
    assert np.all(np.abs(q.medianCNo[[0, 1, 3, 4, 6, 7]] - 50.0) < 1.0)
    assert q[0].CNo.shape == (100,) and q[0].lockPass.dtype == bool
    assert list(t._acq.channels.status) == ['T'] * 8            # the acquisition's channel table is left alone


def test_without_the_detector_nothing_is_computed(monkeypatch, capsys):
    m, ctx, t = _tracked(monkeypatch, False)
    assert ctx.calls == ["track"]
    assert [x.decode() if isinstance(x, bytes) else x for x in t.results.status] == ['T'] * 8
    assert ctx.calls == ["track"]
    q = t.quality                                               # ... until somebody asks
    assert ctx.calls == ["track", "quality"] and np.sum(q.lostAtMs >= 0) == 2
    assert [x.decode() if isinstance(x, bytes) else x for x in t.results.status] == ['T'] * 8
    t.showTrackingQuality()
    out = capsys.readouterr().out
    assert out.count('\n|      ') == 8 and 'Lost at' in out


def test_a_new_track_and_assigned_results_start_afresh(monkeypatch):
    m, ctx, t = _tracked(monkeypatch, False)
    q1 = t.quality
    t.track(m.DeviceFile(type("Rec", (), {"__len__": lambda self: 10 ** 9})()))
    assert t._quality is None
    q2 = t.quality
    assert ctx.calls == ["track", "quality", "track", "quality"] and np.array_equal(q1.lostAtMs, q2.lostAtMs)
    # the reference's cache path: results assigned from an .npy file; the quality reads their I_P / Q_P
    res = t.results
    keep = np.recarray((2,), dtype=res.dtype)
    keep[0], keep[1] = res[2], res[0]
    t.results = keep
    q3 = t.quality
    assert list(q3.PRN) == [3, 1] and q3.lostAtMs[0] == q1.lostAtMs[2] and q3.lostAtMs[1] == -1
    assert np.array_equal(q3[1].CNo, q1[0].CNo, equal_nan=True)
