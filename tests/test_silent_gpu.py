"""Records that go silent, end to end on the GPU: the search on every path it has, the queued step, and every tracking kernel
family, against the oracle on the same arrays (tests/silent_cases.py; tests/test_silent_host.py holds that table against the
oracle alone).  A stretch of exact zeros is the one input on which the reference leaves the finite numbers: the search's metric
is 0 / 0, and tracking dies with ValueError at the block after the first one whose six sums are exactly zero.  The product must
do the same on every kernel: ValueError (SGX_E_SILENT) that names the lowest silent channel and the block that could not start,
with the series written until then.  Run with -m gpu."""
import os

import numpy as np
import pytest

import lock_spec
import replay_spec
import silent_cases as sc
from conftest import pkg
from oracle import softgnss_oracle as orc

pytestmark = pytest.mark.gpu

TRK_TOL = 1e-6       # tests/test_gpu_parity.py: correlator series within 1e-6 max(1, RMS |P|), block boundaries exact
RATE_TOL = (1e-6, 1e-5, 1e-7)   # test_track_golden_via_real_file: codeFreq, carrFreq (Hz), discriminators / NCO commands
METRIC_RTOL = 1e-9   # test_acquire_accepts_any_real_valued_signal
N = sc.N
KEYS = ("carrFreq", "codePhase", "peakMetric", "freqBin", "fineIdx")
INT8_CASES = ("scene", "zeros-int8", "noise-only", "first-ms-silent", "second-ms-silent", "late-signal")
FLOAT_CASES = ("zeros-float64", "zeros-uint8", "nan-sample", "inf-sample")


@pytest.fixture(scope="module")
def m():
    return pkg()


def _settings(m, fs=38192000.0, IF=9548000.0, nch=8, ms=sc.TRACK_MS, dtype=None):
    s = m.Settings()
    s.samplingFreq, s.IF, s.numberOfChannels, s.msToProcess = fs, IF, nch, float(ms)
    if dtype is not None:
        s.dataType = np.dtype(dtype).name
    return s


def _same_search(got, want, idx=None, freq_bin_of=None, what=""):
    """Indices equal, peakMetric NaN where the oracle's is and within METRIC_RTOL elsewhere.  idx: the oracle's entries the
    call searched; freq_bin_of: bool per entry - freqBin is compared only there (arg-maxes clear of a tie)."""
    idx = np.arange(len(got["peakMetric"])) if idx is None else np.asarray(idx)
    w = {k: np.asarray(want[k])[idx] for k in KEYS}
    for k in ("carrFreq", "codePhase", "fineIdx"):
        assert np.array_equal(np.asarray(got[k]), w[k]), (what, k, got[k], w[k])
    sel = np.ones(idx.size, dtype=bool) if freq_bin_of is None else np.asarray(freq_bin_of)[idx]
    assert np.array_equal(np.asarray(got["freqBin"])[sel], w["freqBin"][sel]), (what, got["freqBin"], w["freqBin"])
    assert np.array_equal(np.isnan(got["peakMetric"]), np.isnan(w["peakMetric"])), (what, got["peakMetric"], w["peakMetric"])
    assert np.allclose(got["peakMetric"], w["peakMetric"], rtol=METRIC_RTOL, atol=0, equal_nan=True), \
        (what, got["peakMetric"], w["peakMetric"])


@pytest.fixture(scope="module")
def noise_clear():
    clear = sc.clear_of_a_tie(sc.search_signal("noise-only"))
    print("noise-only: freqBin compared for %d of 32 PRNs" % clear.sum())
    assert clear.sum() >= 24, "choose another seed: a failure of the case, not of the kernel"
    return clear


# ================================ search ================================
@pytest.mark.parametrize("name", INT8_CASES)
def test_search_of_an_int8_record(m, name, noise_clear):
    """sgx_acquire (2 blocks, the reference's rule and the non-coherent sum), sgx_acquire_f64 on the same samples, and
    sgx_acquire_sharded for rank 0 of 8 without a communicator"""
    s = _settings(m)
    ctx = m.engine.get_context(s, 0)
    x = sc.search_signal(name)
    fb = noise_clear if name == "noise-only" else None
    rec = ctx.upload(x)
    try:
        _same_search(ctx.acquire(rec, 0, x.size, list(range(32))), sc.search_expect(name), freq_bin_of=fb, what=name)
        fbn = sc.clear_of_a_tie(x, noncoh=True) if name == "noise-only" else None
        _same_search(ctx.acquire(rec, 0, x.size, list(range(32)), noncoh=True), sc.search_expect(name, "noncoh"),
                     freq_bin_of=fbn, what=name + " noncoh")
        _same_search(ctx.acquire_f64(x, list(range(32))), sc.search_expect(name, "f64"), freq_bin_of=fb, what=name + " f64")
        sh = pkg("shard")
        a = m.AcquisitionResult(s, device=0)
        sh.acquire_sharded(a, m.DeviceSignal(rec, 0, x.size), 0, 8, sh.LocalGather())
        got = dict(carrFreq=a.carrFreq[:4], codePhase=a.codePhase[:4], peakMetric=a.peakMetric[:4],
                   freqBin=a.internals["freqBin"][:4], fineIdx=a.internals["fineIdx"][:4])
        _same_search(got, sc.search_expect(name), idx=range(4), freq_bin_of=fb, what=name + " sharded")
    finally:
        rec.free()


@pytest.mark.parametrize("name", FLOAT_CASES)
def test_search_of_a_float_signal(m, name):
    """sgx_acquire_f64: zeros as float64 and as uint8 bytes of value 0, and the default scene with one NaN, respectively +Inf
    sample in the second block - the reference's NaN metric, freqBin 0, nothing found"""
    s = _settings(m)
    ctx = m.engine.get_context(s, 0)
    x = sc.search_signal(name)
    want = sc.search_expect(name, "f64")
    assert np.isnan(want["peakMetric"]).all()
    for noncoh in (False, True):
        got = ctx.acquire_f64(x, list(range(32)), noncoh=noncoh)
        w = want if not noncoh else sc.search_expect(name, "noncoh")
        _same_search(got, w, what="%s noncoh=%r" % (name, noncoh))
    # the sharded search of a host signal, rank 0 of 8 run alone: sgx_acquire_sharded itself takes a resident int8 record
    # only, so a float signal goes through the rank's share of AcquisitionResult.acquire, packed and merged as a rank's peaks
    sh = pkg("shard")
    b = m.AcquisitionResult(s, device=0)
    sh.acquire_sharded(b, x, 0, 8, sh.LocalGather())
    got = dict(carrFreq=b.carrFreq[:4], codePhase=b.codePhase[:4], peakMetric=b.peakMetric[:4],
               freqBin=b.internals["freqBin"][:4], fineIdx=b.internals["fineIdx"][:4])
    _same_search(got, want, idx=range(4), what=name + " sharded")
    a = m.AcquisitionResult(s, device=0)
    a.acquire(x)                                   # the drop-in class on the same array
    assert np.isnan(a.peakMetric).all() and not a.carrFreq.any()
    a.preRun()
    assert not a.channels.PRN.any() and set(a.channels.status) == {"-"}


@pytest.mark.parametrize("name", INT8_CASES[1:] + FLOAT_CASES)
@pytest.mark.parametrize("noncoh", [False, True], ids=["window-rule", "noncoh"])
def test_coherent_search(m, name, noncoh):
    """sgx_acquire_coherent / _f64, 2 windows of 2 ms, against tests/coherent_acq_spec.py on the same array"""
    s = _settings(m)
    ctx = m.engine.get_context(s, 0)
    x = sc.search_signal(name)
    prns = list(sc.COHERENT_PRNS)
    want = sc.search_expect(name, "coherent-noncoh" if noncoh else "coherent")
    fb = None
    if name == "noise-only":
        import coherent_acq_spec as spec
        fb = np.zeros(32, dtype=bool)
        for p in prns:
            fb[p] = spec.rel_gap(want["details"][p]["bins"]) >= sc.TIE_GAP
    if x.dtype == np.int8:
        rec = ctx.upload(x)
        try:
            got = ctx.acquire_coherent(rec, 0, x.size, prns, coherent_ms=2, n_windows=2, noncoh=noncoh)
        finally:
            rec.free()
    else:
        got = ctx.acquire_coherent_f64(x, prns, coherent_ms=2, n_windows=2, noncoh=noncoh)
    _same_search(got, want, idx=prns, freq_bin_of=fb, what="%s coherent noncoh=%r" % (name, noncoh))


@pytest.mark.parametrize("name", sc.ANY_RATE_CASES)
def test_any_rate_search(m, name):
    """16.3676 Msps: a code period of 16 368 samples is searched on a padded transform, and the block rule runs on the host
    (acq_passes_peaks) - every search case again, on a two-satellite scene of that rate; int8 records also as the non-coherent
    sum and through acquire_f64"""
    s = _settings(m, *sc.ANY_RATE)
    assert s.samplesPerCode == sc.ANY_N
    ctx = m.engine.get_context(s, 0)
    x = sc.any_rate_signal(name)
    want = sc.any_rate_expect(name)
    assert np.isnan(want["peakMetric"]).all() == (name in sc.ALL_NAN), name
    if name in sc.BLOCK_SEL:
        found = np.flatnonzero(want["carrFreq"] > 0)
        assert found.size == 2 and np.all(want["blockSel"][found] == sc.BLOCK_SEL[name])
    fb = fbn = None
    if name == "noise-only":
        fb = sc.clear_of_a_tie(x, fs=sc.ANY_RATE[0], IF=sc.ANY_RATE[1])
        fbn = sc.clear_of_a_tie(x, noncoh=True, fs=sc.ANY_RATE[0], IF=sc.ANY_RATE[1])
        assert fb.sum() >= 24 and fbn.sum() >= 24
    if x.dtype == np.int8:
        rec = ctx.upload(x)
        try:
            _same_search(ctx.acquire(rec, 0, x.size, list(range(32))), want, freq_bin_of=fb, what=name + " any-rate")
            _same_search(ctx.acquire(rec, 0, x.size, list(range(32)), noncoh=True), sc.any_rate_expect(name, True),
                         freq_bin_of=fbn, what=name + " any-rate noncoh")
        finally:
            rec.free()
    _same_search(ctx.acquire_f64(x, list(range(32))), want, freq_bin_of=fb, what=name + " any-rate f64")


# ================================ the queued step ================================
def _step(m, s, rec, deferred):
    a = m.AcquisitionResult(s, device=0, deferred=deferred)
    a.acquire(m.DeviceSignal(rec, 0, sc.SEARCH_MS * N))
    a.preRun()
    t = m.TrackingResult(a, device=0)
    fid = m.DeviceFile(rec)
    t.track(fid)
    return a, t, fid


@pytest.mark.parametrize("name,nch,chains,n_active", [("zeros-int8", 8, False, 0), ("noise-only", 8, True, 0),
                                                      ("late-signal", 8, False, 0), ("scene", 8, True, 8), ("scene", 5, True, 5)])
def test_deferred_step_equals_the_eager_one(m, name, nch, chains, n_active):
    """acquire -> preRun -> track queued against the eager calls on records that give the device preRun its rare branches:
    a NaN metric (zeros, late-signal: the queued sequence must NOT apply, flags & 1) and no detection at all (noise-only: a
    chained launch without one active channel); the default scene with 8 and with 5 channels beside them"""
    s = _settings(m, nch=nch)
    ctx = m.engine.get_context(s, 0)
    host = {"zeros-int8": np.zeros(sc.RECORD_MS * N, dtype=np.int8), "noise-only": sc.noise_record(),
            "late-signal": sc.late_signal_record(), "scene": sc.scene()}[name]
    rec = ctx.upload(host)
    try:
        ae, te, fe = _step(m, s, rec, False)
        ad, td, fd = _step(m, s, rec, True)
        assert not te.chained and td.chained == chains, (name, td.chained)
        assert ad.queued == chains
        assert te.series.shape == td.series.shape == (n_active, 13, sc.TRACK_MS)
        assert np.array_equal(td.series, te.series)
        for f in ("carrFreq", "codePhase", "peakMetric"):
            assert np.array_equal(ad.results[f], ae.results[f], equal_nan=True), f
        assert not ad.queued
        for f in ("freqBin", "fineIdx"):
            assert np.array_equal(ad.internals[f], ae.internals[f]), f
        for f in ("PRN", "acquiredFreq", "codePhase", "status"):
            assert np.array_equal(ad.channels[f], ae.channels[f]), f
        assert len(td.results) == len(te.results) == n_active == int(np.sum(ae.channels.PRN != 0))
        for nm in td.results.dtype.names:
            for j in range(len(te.results)):
                assert np.array_equal(td.results[j][nm], te.results[j][nm]), nm
        want = sc.search_expect(name)
        _same_search({k: ae.results[k] for k in ("carrFreq", "codePhase", "peakMetric")} |
                     {k: ae.internals[k] for k in ("freqBin", "fineIdx")}, want,
                     freq_bin_of=sc.clear_of_a_tie(sc.search_signal(name)) if name == "noise-only" else None, what=name)
        if n_active:
            assert fd.tell() == fe.tell()
    finally:
        rec.free()


# ================================ tracking ================================
def _launch(m, fam, case):
    """The family's launch on the case's record -> (context, record, chans, outcome): outcome (series, ms_done), or the
    SilentChannelError."""
    s = _settings(m, fam.fs, fam.IF, fam.nch, dtype=fam.dtype)
    ctx = m.engine.get_context(s, 0)
    ch = sc.channels(fam.fs, fam.IF, fam.nch)
    phase = sc.start_bytes(fam)
    chans = [(int(ch["PRN"][i]), float(ch["acquiredFreq"][i]), float(phase[i])) for i in range(fam.nch)] * fam.repeat
    rec = ctx.upload_bytes(sc.track_record(case, fam.name))
    code = m.tracking._DT_CODES[fam.dtype.kind + str(fam.dtype.itemsize)]
    before = {k: os.environ.get(k) for k in fam.env}
    os.environ.update(fam.env)
    try:
        try:
            out = ctx.track(rec, chans, sc.TRACK_MS, data_type=code)
        except ValueError as e:
            out = e
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    tm = ctx.timing()
    assert tm["track_kernel"] == fam.kernel, (fam.name, tm["track_kernel"])
    if fam.members is not None:
        assert tm["track_members"] == fam.members, (fam.name, tm["track_members"])
    return ctx, rec, chans, out


def _launch_queued(m, fam, case):
    """The queued step on the case's record (the search reads its first 11 ms, which every case here leaves alone)."""
    s = _settings(m, nch=fam.nch)
    ctx = m.engine.get_context(s, 0)
    rec = ctx.upload(sc.track_record(case, fam.name))
    a = m.AcquisitionResult(s, device=0, deferred=True)
    a.acquire(m.DeviceSignal(rec, 0, sc.SEARCH_MS * N))
    a.preRun()
    t = m.TrackingResult(a, device=0)
    try:
        t.track(m.DeviceFile(rec))
        out = (t.series, np.full(fam.nch, sc.TRACK_MS))
    except ValueError as e:
        out = e
    assert a.queued, "the queued sequence applied: nobody has looked at the search"
    if isinstance(out, Exception):                      # sgx_track_chained hands the table over with the error
        prn, freq, cph, n_act = out.table
        ch0 = sc.channels()
        assert n_act == fam.nch and np.array_equal(prn, ch0["PRN"]) and np.array_equal(cph, ch0["codePhase"])
        assert np.array_equal(freq, ch0["acquiredFreq"])
    assert ctx.timing()["track_kernel"] == fam.kernel
    ch = sc.channels()
    assert np.array_equal(a.channels.PRN, ch["PRN"]) and np.array_equal(a.channels.codePhase, ch["codePhase"])
    return ctx, rec, None, out


def _check_channel(got, done, e, c, what):
    """Channel c's rows against the oracle's: rows < k to TRK_TOL with block boundaries exact, row k zeros and NaN where the
    oracle has them, the rows behind it the pre-fill of tracking.py:65-94, ms_done = k + 1."""
    want, k = e["rows"], e["k"]
    n = want.shape[1]                                         # k + 1, or all TRACK_MS
    assert done == n, (what, c, done, n)
    assert np.array_equal(got[0, :n], want[0]), (what, c, "absoluteSample")
    fin = n if k is None else k
    scale = max(1.0, float(np.sqrt(np.mean(want[3, :fin] ** 2 + want[7, :fin] ** 2)))) if fin else 1.0
    err = float(np.max(np.abs(got[3:9, :fin] - want[3:9, :fin]), initial=0.0)) / scale
    assert err < TRK_TOL, (what, c, err)
    assert np.isfinite(got[:, :fin]).all()
    # the rates and the discriminators of every finite block - the partly silent one, whose reduced sums they see, among them
    # (a wrong value there cannot show later: the next block's sums are zero whatever its length); test_gpu_parity.py's bounds
    for rows, bound, name in ((slice(1, 2), RATE_TOL[0], "codeFreq"), (slice(2, 3), RATE_TOL[1], "carrFreq"),
                              (slice(9, 13), RATE_TOL[2], "discriminators / NCO commands")):
        d = float(np.max(np.abs(got[rows, :fin] - want[rows, :fin]), initial=0.0))
        assert d < bound, (what, c, name, d)
    if k is None:
        return err
    assert np.all(got[3:9, k] == 0.0), (what, c, got[3:9, k])
    assert np.isnan(got[[1, 2, 9, 10, 11, 12], k]).all(), (what, c, got[:, k])
    assert np.all(got[[0, 3, 4, 5, 6, 7, 8], k + 1:] == 0.0) and np.all(got[[1, 2, 9, 10, 11, 12], k + 1:] == np.inf), (what, c)
    return err


# (the queued step searches the record it tracks: with the first tracked sample silent nothing is found - that is late-signal
# of test_deferred_step_equals_the_eager_one)
TRACK_RUNS = [(c, f.name) for c in sorted(sc.TRACKING) for f in sc.FAMILIES if not (f.chained and c == "silent-from-start")]


@pytest.mark.parametrize("case,family", TRACK_RUNS, ids=["%s-%s" % r for r in TRACK_RUNS])
def test_tracking_a_record_that_goes_silent(m, case, family):
    fam = sc.FAMILY[family]
    exp = sc.track_expect(case, family)
    what = "%s / %s" % (case, family)
    ctx, rec, chans, out = (_launch_queued if fam.chained else _launch)(m, fam, case)
    try:
        first = sc.first_silent(case, family)
        if case in sc.MUST_RAISE:
            assert first is not None
            assert isinstance(out, ValueError), (what, "completed")
            text = str(out)
            print("%s: %s" % (what, text))
            assert isinstance(out, m._native.SilentChannelError) and not isinstance(out, m._native.SgxError)
            assert "cannot convert float NaN to integer" in text
            assert ("channel %d went silent" % first[0]) in text and ("block %d has no length" % (first[1] + 1)) in text
            assert "Not able to read" not in text and "dllNoiseBandwidth" not in text
            series, done = out.series, out.ms_done
        else:
            assert first is None and not isinstance(out, Exception), (what, out)
            series, done = out
        assert series.shape[1:] == (13, sc.TRACK_MS)
        worst = 0.0
        for c, e in enumerate(exp):
            worst = max(worst, _check_channel(series[c], int(done[c]), e, c, what))
        print("%s: correlator series within %.2e of the oracle (bar %.0e)" % (what, worst, TRK_TOL))
        for i in range(fam.nch, fam.nch * fam.repeat):                       # replicated channels: the same rows
            assert done[i] == done[i % fam.nch] and np.array_equal(series[i], series[i % fam.nch], equal_nan=True), (what, i)
    finally:
        rec.free()


def test_the_drop_in_class_raises_the_references_exception(m, capsys):
    """TrackingResult.track on a file object: ValueError, never the short-read message - the record did not run out"""
    fam = sc.FAMILY["trk3"]
    s = _settings(m)
    ch = sc.channels()
    a = m.AcquisitionResult(s, device=0)
    a._channels = np.rec.fromarrays([ch["PRN"], ch["acquiredFreq"], ch["codePhase"], ["T"] * 8],
                                    names="PRN,acquiredFreq,codePhase,status")
    ctx = m.engine.get_context(s, 0)
    rec = ctx.upload(sc.track_record("silent-from-k", fam.name))
    t = m.TrackingResult(a, device=0)
    fid = m.DeviceFile(rec)
    try:
        with pytest.raises(ValueError, match="channel 0 went silent .* block 14 has no length"):
            t.track(fid)
        assert not t.has_results() and "Not able to read" not in capsys.readouterr().out
    finally:
        rec.free()


# ================================ downstream ================================
def test_quality_and_replay_of_a_channel_that_went_silent(m):
    """The series of silent-from-k with ms_done = k + 1 through sgx_track_quality (tests/lock_spec.py) and sgx_track_replay
    (tests/replay_spec.py); with every row taken as tracked the replay refuses (the recorded rates give no block)"""
    fam = sc.FAMILY["trk3"]
    ctx, rec, chans, out = _launch(m, fam, "silent-from-k")
    try:
        assert isinstance(out, m._native.SilentChannelError)
        series, done = np.array(out.series), np.array(out.ms_done)
        assert list(done) == [e["k"] + 1 for e in sc.track_expect("silent-from-k", "trk3")]
        p = m._native.lock_params(_settings(m))
        p.window, p.max_fail = 7, 2
        for md in (done, None):
            cno, cl, ok, lost = ctx.track_quality(series[:, 3], series[:, 7], p, ms_done=md)
            wc, wl, wp, wlost = lock_spec.quality(series[:, 3], series[:, 7], p.T, p.cno_min, p.carr_lock_min, p.window,
                                                  p.max_fail, md)
            assert np.array_equal(np.isnan(cno), np.isnan(wc)) and np.allclose(cno, wc, rtol=0, atol=1e-9, equal_nan=True)
            assert np.array_equal(np.isnan(cl), np.isnan(wl)) and np.allclose(cl, wl, rtol=0, atol=1e-12, equal_nan=True)
            assert np.array_equal(ok, wp) and np.array_equal(lost, wlost), (lost, wlost)
            assert not ok[np.isnan(cno)].any()                       # a window without power fails
        assert np.all(lost >= 0)                                     # (all rows: windows 2 and 3 hold the pre-fill only)
        taps = [-0.5, 0.0, 0.5]
        got = ctx.track_replay(rec, chans, series, taps, ms_done=done)
        want, _ = replay_spec.replay_channels(sc.oracle_settings(), sc.track_record("silent-from-k", "trk3"), "int8", chans,
                                              series, done, taps)
        for c in range(fam.nch):
            assert np.max(np.abs(got[c] - want[c])) <= replay_spec.bar(series[c, 3, :done[c] - 1], series[c, 7, :done[c] - 1])
            assert np.all(got[c, :, :, done[c] - 1:] == 0.0)         # the silent block correlates to zero, the rest is unset
        with pytest.raises(m._native.SgxError, match="give no block"):
            ctx.track_replay(rec, chans, series, taps)
    finally:
        rec.free()
