"""C/N0 estimate and lock detector on the GPU (sgx_track_quality, csrc/sgx_quality.hip): the kernel against the numpy
contract of tests/lock_spec.py, known answers on the synthetic scene, a satellite that vanishes, a channel without a
signal, the many-channel shape, the input forms, the queued step and the argument checks.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import lock_spec as spec
from conftest import pkg

pytestmark = pytest.mark.gpu

MS = 4000
SPLIT_MS = 2000
GONE_PRN = 11            # amplitude 7 in Scene.default: set to 0 from SPLIT_MS on


def _status(res):
    return [x.decode() if isinstance(x, bytes) else x for x in res.status]


def _settings(m, ms=MS, lock=False):
    s = m.Settings()
    s.msToProcess = float(ms)
    s.lockDetector = lock
    return s


def _track(m, s, rec, deferred=False):
    n = s.samplesPerCode
    a = m.AcquisitionResult(s, device=0, deferred=deferred)
    a.acquire(m.DeviceSignal(rec, 0, 11 * n))
    a.preRun()
    t = m.TrackingResult(a, device=0)
    t.track(m.DeviceFile(rec))
    return a, t


@pytest.fixture(scope="module")
def scene_run():
    """The default scene, 8 channels x 4 000 ms, tracked from a record generated in HBM."""
    m = pkg()
    s = _settings(m)
    ctx = m.engine.get_context(s, 0)
    sc = m.synth.Scene.default()
    rec = ctx.synth(sc, m.synth.record_length(s.samplesPerCode, MS))
    a, t = _track(m, s, rec)
    assert t.series.shape == (8, 13, MS)
    yield m, s, ctx, sc, rec, a, t
    rec.free()


@pytest.fixture(scope="module")
def spliced(scene_run):
    """The default scene whose satellite GONE_PRN is switched off at SPLIT_MS: the same seed with that amplitude 0, so
    the noise and the other satellites continue unchanged across the splice."""
    m, s, ctx, sc, rec, a, t = scene_run
    sats = [dict(x, amp=0 if x["prn"] == GONE_PRN else x["amp"]) for x in sc.sats]
    sc2 = m.synth.Scene(sc.seed, sats, sc.fs)
    n = m.synth.record_length(s.samplesPerCode, MS)
    rec2 = ctx.synth(sc2, n)
    cut = int(SPLIT_MS * 1e-3 * s.samplingFreq)
    host = np.concatenate([rec.download(0, cut), rec2.download(cut, n - cut)])
    rec2.free()
    both = ctx.upload(host)
    yield both
    both.free()


def _compare(got, want, cno_min, carr_min):
    """Kernel (cno, carr, pass, lost) against the numpy contract: values to 1e-9 dB / 1e-12; pass and lost identical
    except at a window whose value lies within those tolerances of a threshold."""
    gc, gl, gp, glost = got
    wc, wl, wp, wlost = want
    assert gc.shape == wc.shape and gp.dtype == bool
    fin = np.isfinite(wc)
    assert np.array_equal(fin, np.isfinite(gc)) and np.array_equal(np.isnan(wc), np.isnan(gc))
    assert np.array_equal(gc[~fin & ~np.isnan(wc)], wc[~fin & ~np.isnan(wc)])           # +-inf where the contract has them
    assert np.max(np.abs(gc[fin] - wc[fin]), initial=0.0) < 1e-9
    assert np.array_equal(np.isnan(wl), np.isnan(gl))
    assert np.max(np.abs(np.nan_to_num(gl - wl)), initial=0.0) < 1e-12
    edge = (np.abs(wc - cno_min) < 1e-9) | (np.abs(wl - carr_min) < 1e-12)
    assert np.array_equal(gp[~edge], wp[~edge])
    for c in range(len(wlost)):
        if not np.any(edge[c]):
            assert glost[c] == wlost[c], (c, glost[c], wlost[c])


def _spec(i_p, q_p, p, ms_done=None):
    return spec.quality(i_p, q_p, p.T, p.cno_min, p.carr_lock_min, p.window, p.max_fail, ms_done)


@pytest.mark.parametrize("window,max_fail", [(20, 25), (2, 7), (37, 3), (2500, 1)])
def test_kernel_against_the_contract(scene_run, window, max_fail):
    """Window lengths from 2 ms to one longer than the LDS stretch (read from HBM), and channels cut short by ms_done."""
    m, s, ctx, sc, rec, a, t = scene_run
    p = m._native.lock_params(s)
    p.window, p.max_fail = window, max_fail
    i_p, q_p = t.series[:, 3], t.series[:, 7]
    got = ctx.track_quality(i_p, q_p, p)
    _compare(got, _spec(i_p, q_p, p), p.cno_min, p.carr_lock_min)
    done = np.array([MS, 0, 1, window - 1, window, min(2 * window + 1, MS), MS - 1, 2600], dtype=np.int32)
    got = ctx.track_quality(i_p, q_p, p, ms_done=done)
    want = _spec(i_p, q_p, p, done)
    _compare(got, want, p.cno_min, p.carr_lock_min)
    assert np.all(np.isnan(got[0][1])) and not np.any(got[2][1]) and got[3][1] == -1
    # a strict threshold: every window fails, every channel is lost at window max_fail - 1 (if it has that many)
    p.cno_min = 200.0
    got = ctx.track_quality(i_p, q_p, p, ms_done=done)
    _compare(got, _spec(i_p, q_p, p, done), p.cno_min, p.carr_lock_min)
    assert got[3][0] == max_fail - 1


def _expected_cno(sc, fs, rc=1.023e6):
    """C/N0 of each satellite from the generator's constants (synth.py): amplitude A 127/128 after the cosine table; the
    Irwin-Hall noise term (four bytes, centred, x 35 / 256: 408 LSB^2), white over fs / 2; the other satellites' power
    A^2 / 2 as noise at the spectral separation of two BPSK signals of chip rate rc, kappa = 2 / (3 rc).  That is
    A^2 / 2 / N0 with N0 = 2 var / fs + kappa sum_o A_o^2 / 2; counted as white noise instead (kappa = 2 / fs), the other
    satellites would read ~12 times weaker than they are (fs kappa / 2 = 12.4 at 38.192 MHz) and every C/N0 ~6 dB higher."""
    g = 127.0 / 128.0
    var_n = 4 * (256 ** 2 - 1) / 12.0 * (35.0 / 256.0) ** 2 + 1.0 / 12.0
    kappa = 2.0 / (3.0 * rc)
    amps = np.array([x["amp"] for x in sc.sats], dtype=np.float64) * g
    out = {}
    for k, x in enumerate(sc.sats):
        n0 = 2.0 * var_n / fs + kappa * (np.sum(amps ** 2) - amps[k] ** 2) / 2.0
        out[x["prn"]] = 10 * np.log10(amps[k] ** 2 / 2.0 / n0)
    return out, {x["prn"]: x["amp"] for x in sc.sats}


@pytest.fixture(scope="module")
def full_scene():
    """The default scene over the full 37 000 ms (BASELINE config 3's run)."""
    m = pkg()
    s = _settings(m, ms=37000)
    ctx = m.engine.get_context(s, 0)
    sc = m.synth.Scene.default()
    rec = ctx.synth(sc, m.synth.record_length(s.samplesPerCode, 37000))
    a, t = _track(m, s, rec)
    rec.free()
    return m, s, sc, t


def test_known_answer_on_the_default_scene(full_scene):
    """Over the full 37 s: the other satellites' share of the noise is a cross-correlation whose relative code phase
    drifts by (Doppler difference / 1540) chips per second, so it stays put for seconds and the median of one 4-s run
    carries its state (the amplitude-8 and -6 classes then differ by 3.8 dB on the default scene's first 4 s, 3.0 dB over
    37 s, 2.8 dB expected)."""
    m, s, sc, t = full_scene
    want, amp = _expected_cno(sc, s.samplingFreq)
    assert abs(want[1] - 54.1) < 0.1 and abs(want[7] - 51.3) < 0.1
    q = t.quality
    assert len(q) == 8 and sorted(q.PRN) == sorted(want)
    for r in q:
        assert abs(r.medianCNo - want[int(r.PRN)]) < 1.5, (int(r.PRN), r.medianCNo, want[int(r.PRN)])
        assert r.lostAtMs == -1
        assert np.median(r.carrLock) >= 0.95
    med = {int(r.PRN): r.medianCNo for r in q}
    hi = np.mean([med[p] for p in med if amp[p] == 8])
    lo = np.mean([med[p] for p in med if amp[p] == 6])
    exp = np.mean([want[p] for p in med if amp[p] == 8]) - np.mean([want[p] for p in med if amp[p] == 6])
    assert abs((hi - lo) - exp) < 0.7, (hi - lo, exp)
    assert _status(t.results) == ['T'] * 8


def test_a_satellite_that_vanishes_is_declared_lost(scene_run, spliced):
    m = pkg()
    s = _settings(m, lock=True)
    a, t = _track(m, s, spliced)
    q = t.quality
    prn = [int(p) for p in q.PRN]
    assert GONE_PRN in prn and len(prn) == 8
    for j, r in enumerate(q):
        if prn[j] == GONE_PRN:
            assert SPLIT_MS < r.lostAtMs <= 3500, r.lostAtMs
        else:
            assert r.lostAtMs == -1, (prn[j], r.lostAtMs)
    assert _status(t.results) == ['-' if p == GONE_PRN else 'T' for p in prn]
    s2 = _settings(m, lock=False)
    a2, t2 = _track(m, s2, spliced)
    assert _status(t2.results) == ['T'] * 8
    assert np.array_equal(t2.series, t.series)


def test_a_channel_on_an_absent_prn_is_lost(scene_run):
    m, s, ctx, sc, rec, a, t = scene_run
    absent = [p for p in (9, 28, 2) if p not in [x["prn"] for x in sc.sats]]
    chans = [(absent[0], s.IF + 321.0, 17.0), (absent[1], s.IF - 2750.0, 30011.0)]
    series, done = ctx.track(rec, chans, 2000)
    assert np.all(done == 2000)
    cno, cl, ok, lost = ctx.track_quality(series[:, 3], series[:, 7], m._native.lock_params(s))
    assert np.all(lost >= 0) and np.all((lost + 1) * 20 <= 1500), lost


def test_many_channels_at_staggered_offsets(scene_run):
    """1 024 throughput-mode channels x 500 ms started whole code periods apart; and 3 072 channels of 500 ms."""
    m, s, ctx, sc, rec, a, t = scene_run
    n = s.samplesPerCode
    chans = [(int(c.PRN), float(c.acquiredFreq), float(c.codePhase)) for c in a.channels]
    many = [(chans[i % 8][0], chans[i % 8][1], chans[i % 8][2] + (i // 8) * n) for i in range(1024)]
    series, done = ctx.track(rec, many, 500)
    assert np.all(done == 500)
    p = m._native.lock_params(s)
    got = ctx.track_quality(series[:, 3], series[:, 7], p)
    _compare(got, _spec(series[:, 3], series[:, 7], p), p.cno_min, p.carr_lock_min)
    i3, q3 = np.tile(series[:, 3], (3, 1)), np.tile(series[:, 7], (3, 1))
    got3 = ctx.track_quality(i3, q3, p)
    assert got3[0].shape == (3072, 25)
    for k in range(4):
        assert np.array_equal(got3[k], np.concatenate([got[k]] * 3), equal_nan=True)


def test_input_forms_give_identical_outputs(scene_run):
    m, s, ctx, sc, rec, a, t = scene_run
    p = m._native.lock_params(s)
    pinned = t.series                                       # pinned_empty: the array track() returns
    pageable = np.array(pinned)
    outs = [ctx.track_quality(pinned[:, 3], pinned[:, 7], p),
            ctx.track_quality(pageable[:, 3], pageable[:, 7], p),
            ctx.track_quality(np.ascontiguousarray(pinned[:, 3]), np.ascontiguousarray(pinned[:, 7]), p),
            ctx.track_quality(pageable[:, 3], np.ascontiguousarray(pageable[:, 7]), p)]
    for o in outs[1:]:
        for k in range(4):
            assert np.array_equal(o[k], outs[0][k], equal_nan=True)


def test_the_queued_step_gives_the_same_quality(spliced):
    m = pkg()
    s = _settings(m, lock=True)
    ae, te = _track(m, s, spliced, deferred=False)
    ad, td = _track(m, s, spliced, deferred=True)
    assert td.chained and not te.chained
    assert _status(td.results) == _status(te.results) and '-' in _status(te.results)
    qe, qd = te.quality, td.quality
    for name in ("PRN", "lostAtMs", "medianCNo"):
        assert np.array_equal(qe[name], qd[name], equal_nan=True), name
    for j in range(len(qe)):
        for name in ("CNo", "carrLock", "lockPass"):
            assert np.array_equal(qe[j][name], qd[j][name], equal_nan=True), name


def test_bad_arguments_are_refused(scene_run):
    m, s, ctx, sc, rec, a, t = scene_run
    n = m._native
    i_p, q_p = np.ascontiguousarray(t.series[:, 3, :100]), np.ascontiguousarray(t.series[:, 7, :100])
    good = n.lock_params(s)

    def params(**kw):
        p = n.LockParams(good.T, good.cno_min, good.carr_lock_min, good.window, good.max_fail)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    for kw in (dict(window=1), dict(window=101), dict(max_fail=0), dict(T=0.0), dict(T=-1e-3), dict(T=float("inf")),
               dict(T=float("nan"))):
        with pytest.raises(n.SgxError) as e:
            ctx.track_quality(i_p, q_p, params(**kw))
        assert e.value.code == n.SGX_E_ARG, kw
    for done in ([100] * 7 + [101], [-1] + [100] * 7):
        with pytest.raises(n.SgxError) as e:
            ctx.track_quality(i_p, q_p, good, ms_done=done)
        assert e.value.code == n.SGX_E_ARG
    out = [np.zeros((8, 5)), np.zeros((8, 5)), np.zeros((8, 5), dtype=np.uint8), np.zeros(8, dtype=np.int32)]
    ptrs = [o.ctypes.data_as(C.c_void_p) for o in out]
    ip = i_p.ctypes.data_as(C.c_void_p)
    qp = q_p.ctypes.data_as(C.c_void_p)
    L = n.lib()
    assert L.sgx_track_quality(ctx._h, ip, qp, 99, 8, 100, None, C.byref(good), *ptrs) == n.SGX_E_ARG   # row_stride < ms
    assert L.sgx_track_quality(ctx._h, None, qp, 100, 8, 100, None, C.byref(good), *ptrs) == n.SGX_E_ARG
    assert L.sgx_track_quality(ctx._h, ip, qp, 100, 8, 100, None, None, *ptrs) == n.SGX_E_ARG
    assert L.sgx_track_quality(ctx._h, ip, qp, 100, 8, 100, None, C.byref(good), *(ptrs[:3] + [None])) == n.SGX_E_ARG
    assert L.sgx_track_quality(ctx._h, ip, qp, 100, 8, 100, None, C.byref(good), *ptrs) == n.SGX_OK
