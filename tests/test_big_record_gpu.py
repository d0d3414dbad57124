"""Records longer than 4 GiB on every path that reads one: the record handle, the generator, the record stages, the probe and
the monitor, the acquisition entry points, the tracking kernels, the replay and the strong-signal cancellation, each with
record positions beyond 2^31 and 2^32.  Every expectation is a window or an exact integer from tests/big_record.py, whose
rule - a wrap must be visible - is run on the CPU before anything is compared with the device.  The cost is two 4.3 GB
records in HBM (one made there, one uploaded once), the stages' outputs of that size while their test runs (the
cancellation's two calls: two of them) and milliseconds of kernels; nothing on the host grows with the record.  Run with
-m gpu.

Left out on purpose: the float32 sums of requant_stats (taken in double in a fixed order that the contract does not restate;
its counts and max_abs are exact and are compared); the decimator, whose own file holds its 4 GiB case."""
import os
import shutil

import numpy as np
import pytest

import big_record as big
import coh_track_spec as coh_spec
import coherent_acq_spec
import replay_spec
import waterfall_spec
from conftest import pkg
from oracle import softgnss_oracle as orc
from test_coh_track_gpu import _same as _same_as_the_contract

pytestmark = pytest.mark.gpu

B = big.B32
SPC = big.SPC
FS_MHZ = 38.192
PSD_TOL = 1e-9          # tests/test_gpu_parity.py (probeData parity) and tests/test_waterfall_gpu.py
TRK_TOL = 1e-6          # tests/test_gpu_parity.py: the correlator series' bar, 1e-6 max(1, RMS |P|)


@pytest.fixture(scope="module")
def env():
    m = pkg()
    s = m.Settings()
    return m, s, m.engine.get_context(s, 0)


@pytest.fixture(scope="module")
def tiled(env):
    """The tiled record, uploaded once; the host copy is let go at once."""
    m, s, ctx = env
    rec = big.Tiled()
    host = rec.build()
    dev = ctx.upload(host)
    del host
    yield rec, dev
    dev.free()


@pytest.fixture(scope="module")
def scene8(env):
    """The default scene, 2^32 + 100 code periods, made on the device."""
    m, s, ctx = env
    sc = m.synth.Scene.default()
    dev = ctx.synth(sc, big.SCENE_N)
    ctx.sync()
    yield sc, dev, big.scene_reader(m.synth.generate, sc)
    dev.free()


def _report(capsys, what):
    with capsys.disabled():
        print("\n[big record] " + what)


def _trk_err(got, want):
    """tests/test_gpu_parity.py: max |delta| of the six correlator series over max(1, RMS sqrt(I_P^2 + Q_P^2)) per channel."""
    errs = []
    for c in range(want.shape[0]):
        scale = max(1.0, float(np.sqrt(np.mean(want[c, 3] ** 2 + want[c, 7] ** 2))))
        errs.append(np.max(np.abs(got[c, 3:9] - want[c, 3:9])) / scale)
    return max(errs)


# ---- the record handle --------------------------------------------------------------------------------------------------

def test_download_of_windows_beyond_the_boundaries(tiled):
    rec, dev = tiled
    assert len(dev) == rec.n == B + big.EXTRA32
    for w in ((0, 4096), (B // 2 - 2048, B // 2 + 2048), (B - 2048, B + 2048), (rec.n - 4096, rec.n)):
        want = big.wrap_visible(rec.at, big.identity, w)
        assert dev.download(w[0], w[1] - w[0]).tobytes() == want.tobytes(), w


def test_the_device_generator_beyond_the_boundaries(env, scene8):
    m, s, ctx = env
    sc, dev, at = scene8
    assert len(dev) == big.SCENE_N
    for w0, w1 in big.SYNTH_WINDOWS:
        want = big.wrap_visible(at, big.identity, (w0, w1))
        assert dev.download(w0, w1 - w0).tobytes() == want.tobytes(), (w0, w1)
    off, n = big.SYNTH_CALL                                    # a record that BEGINS past 2^32 of the scene
    want = big.wrap_visible(at, big.identity, (off, off + n))
    part = ctx.synth(sc, n, offset=off)
    try:
        assert part.download().tobytes() == want.tobytes()
        assert dev.download(off, n).tobytes() == want.tobytes()
    finally:
        part.free()


def test_a_sparse_file_longer_than_4_gib(env, tmp_path):
    """upload_file and open_file of a file truncated to 2^32 + tail with three written windows: the windows come back, the
    length is right, a window of the hole is zeros."""
    m, s, ctx = env
    free = shutil.disk_usage(str(tmp_path)).free
    if free < 5 * 10 ** 9:
        pytest.skip("the temporary file system has %.1f GB free, the 4.3 GB file wants 5" % (free / 1e9))
    n = B + big.FILE_TAIL
    rng = np.random.default_rng(77)
    path = str(tmp_path / "sparse.bin")
    written = []
    with open(path, "wb") as fh:
        fh.truncate(n)
        for w0, w1 in big.FILE_WINDOWS + ((n - 5000, n),):
            data = rng.integers(-128, 128, w1 - w0).astype(np.int8)
            data[data == 0] = 1
            big.wrap_visible(big.sparse_reader(n, w0, data), big.identity, (w0, w1), sparse=True)
            fh.seek(w0)
            fh.write(data.tobytes())
            written.append((w0, w1, data))
    assert os.path.getsize(path) == n
    for opener, skip in ((ctx.upload_file, 0), (ctx.open_file, 4096)):
        rec = opener(path, skip, n - skip)
        try:
            assert len(rec) == n - skip
            rec.wait()
            for w0, w1, data in written:
                assert rec.download(w0 - skip, w1 - w0).tobytes() == data.tobytes(), (opener.__name__, w0)
            assert not rec.download(B + 3000 - skip + 100, 4096).any()          # the hole behind the window across 2^32
            assert not rec.download(B // 2 + 3000 - skip + 100, 4096).any()
        finally:
            rec.free()


# ---- the record stages on the tiled record ------------------------------------------------------------------------------

def _check_stage(capsys, name, stage, rec, launch, tile_bytes, extra=()):
    """The windows (through the rule, on the CPU first) and the exact counters of one stage's output."""
    assert stage.width >= 2 * tile_bytes, (name, stage.width, tile_bytes)
    windows = stage.windows(rec)
    assert len(windows) >= 4
    wants = [(w, big.wrap_visible(rec.at, stage.contract(rec.n), w)) for w in windows]
    counters = stage.counters(rec)
    out = launch()
    try:
        assert len(out) == stage.out_len(rec.n), name
        for (w0, w1), want in wants:
            got = out.download(w0, w1 - w0)
            assert got.tobytes() == want.tobytes(), \
                "%s: window [%d, %d) differs first at output byte %d" % (name, w0, w1, w0 + int(np.flatnonzero(got != want)[0]))
        for k in sorted(counters):
            if hasattr(out, k):
                assert getattr(out, k) == counters[k], (name, k, getattr(out, k), counters[k])
        for k in extra:
            assert hasattr(out, k) and 0 < counters[k] < len(out), (name, k)
    finally:
        out.free()
    _report(capsys, "%s: %d windows of %d bytes byte for byte (bar: exact), the last at output byte %d; counters %s exact"
            % (name, len(windows), stage.width, windows[-1][0], dict((k, counters[k]) for k in extra)))
    return counters


@pytest.fixture(scope="module")
def cases(tiled):
    return big.stage_cases(tiled[0])


def test_filter_record(env, tiled, cases, capsys):
    m, s, ctx = env
    stage, rec = cases["filter_record"]
    assert stage.h.size == 255 and stage.S == 14
    _check_stage(capsys, "filter_record", stage, rec, lambda: ctx.filter_record(tiled[1], stage.h, stage.S), 4096)


def test_iq_to_if(env, tiled, cases, capsys):
    m, s, ctx = env
    stage, rec = cases["iq_to_if"]
    assert stage.h.size == 63 and stage.flags == 3
    _check_stage(capsys, "iq_to_if", stage, rec,
                 lambda: ctx.iq_to_if(tiled[1], stage.h, stage.S, q_first=True, offset_binary=True), m._native.iq_tile())


def test_requantize_int16(env, tiled, cases, capsys):
    m, s, ctx = env
    stage, rec = cases["requantize_int16"]
    want = _check_stage(capsys, "requantize int16", stage, rec,
                        lambda: ctx.requantize(tiled[1], np.int16, stage.gain["mult"], stage.gain["shift"]),
                        m._native.requant_tile(), ("clipped",))
    got = ctx.requant_stats(tiled[1], np.int16)
    assert got["n_finite"] == want["n_finite"] == rec.n // 2 and got["n_nonfinite"] == 0
    assert got["sum"] == float(want["sum"]) and got["sum_sq"] == float(want["sum_sq"]) and got["max_abs"] == stage.max_abs(rec)
    # an element window that straddles byte 2^32 (element 2^31) and several blocks
    off, count = B // 2 - 2 * rec.P - 12345, 2 * rec.P + 12345 + 40000
    assert 2 * off < B < 2 * (off + count) <= rec.n
    part = big.requant_counts(big.wrap_visible(rec.at, big.identity, (2 * off, 2 * (off + count))), np.int16)
    got = ctx.requant_stats(tiled[1], np.int16, off, count)
    assert got["n_finite"] == count and got["sum"] == float(part["sum"]) and got["sum_sq"] == float(part["sum_sq"])
    _report(capsys, "requant_stats int16: n_finite, sum, sum_sq, max_abs of the whole record and of a window across 2^32 exact")


def test_requantize_float32(env, tiled, cases, capsys):
    m, s, ctx = env
    stage, rec = cases["requantize_float32"]
    want = _check_stage(capsys, "requantize float32", stage, rec,
                        lambda: ctx.requantize(tiled[1], np.float32, scale=stage.gain["scale"]), m._native.requant_tile(),
                        ("clipped",))
    got = ctx.requant_stats(tiled[1], np.float32)
    assert (got["n_finite"], got["n_nonfinite"]) == (want["n_finite"], want["n_nonfinite"]) and want["n_nonfinite"] > 0
    assert got["max_abs"] == stage.max_abs(rec)
    _report(capsys, "requant_stats float32: n_finite, n_nonfinite, max_abs exact; the float sums are not compared")


@pytest.mark.parametrize("name", ["condition_int8", "condition_int16"])
def test_condition(env, tiled, cases, capsys, name):
    m, s, ctx = env
    stage, rec = cases[name]
    got = ctx.cond_stats(tiled[1], stage.dtype, stage.lanes, stage.block, stage.blank_q4)
    want = stage.record_stats(rec)
    assert got.size == want.size > (B // stage.unit) and int(want["n"][-1]) < stage.block       # the last block is partial
    for f in want.dtype.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, "%s: cond_stats.%s differs first at block %d of %d" % (name, f, int(bad[0]), want.size)
    plan = stage.record_plan(rec)
    assert plan.size == want.size
    _check_stage(capsys, name, stage, rec,
                 lambda: ctx.condition(tiled[1], stage.dtype, stage.lanes, stage.block, plan, stage.guard),
                 m._native.cond_tile() * stage.lanes, ("blanked", "clipped"))


def test_resample_16_1_output_beyond_the_boundary(env, cases, capsys):
    """The first 2^28 + 16384 bytes of the tiled record, uploaded separately: the output passes 2^32 while the input index is
    small."""
    m, s, ctx = env
    stage, rec = cases["resample_16_1"]
    assert rec.n == (B >> 4) + 16384 and stage.out_len(rec.n) > B + stage.width
    dev = ctx.upload(rec.build())
    try:
        _check_stage(capsys, "resample 16/1", stage, rec, lambda: ctx.resample(dev, stage.h, stage.S, 16, 1),
                     m._native.resamp_tile(), ("clipped",))
    finally:
        dev.free()


def test_resample_4_3_input_beyond_the_boundary(env, tiled, cases, capsys):
    m, s, ctx = env
    stage, rec = cases["resample_4_3"]
    assert stage.out_len(rec.n) > 5.7e9
    _check_stage(capsys, "resample 4/3", stage, rec, lambda: ctx.resample(tiled[1], stage.h, stage.S, 4, 3),
                 m._native.resamp_tile() * 4 // 16, ("clipped",))


# ---- the strong-signal cancellation ----------------------------------------------------------------------------------------

def test_cancel_across_the_boundaries(env, tiled, capsys):
    """One if_cancel over the whole tiled record at rec_file_offset 0 with the four hand-made channels of big.CancelPlan:
    blocks across 2^31, across 2^32 - one of them starting exactly at 2^32 -, up to the record's last sample and in the
    first tile.  Every channel's window equals its contract under the rule of cancel_cases.compare, the two windows that no
    block touches (across 2^31 + 2^20 and 2^32 - 2^20) are the input, the clip count is the sum of the windows' (only
    covered samples count: exact), the input is not written, and a second call gives the same bytes."""
    m, s, _ = env
    rec, dev = tiled
    plan = big.CancelPlan(rec)
    ctx = m.engine.get_context(plan.s, 0)
    wants = []
    for i, w in enumerate(plan.windows):
        big.wrap_visible(rec.at, plan.contract(i), w)
        wants.append(plan.expect(rec.at, i, *w))
    quiet = [big.wrap_visible(rec.at, big.identity, w) for w in plan.quiet]
    total = sum(e[2] for e in wants)
    assert all(e[2] > 0 for e in wants)
    out = ctx.if_cancel(dev, plan.chans, plan.series, plan.amp, ms_done=plan.ms_done)
    try:
        assert len(out) == rec.n
        got = [out.download(w0, w1 - w0) for w0, w1 in plan.windows]
        excluded = [big.cancel_cases.compare_to(e, "channel %s" % k, y) for e, k, y in zip(wants, plan.names, got)]
        for (w0, w1), want in zip(plan.quiet, quiet):
            assert out.download(w0, w1 - w0).tobytes() == want.tobytes(), (w0, w1)
        assert out.clipped == total, (out.clipped, total)
        for w0, w1 in plan.windows + plan.quiet:
            assert dev.download(w0, w1 - w0).tobytes() == rec.at(w0, w1).tobytes(), (w0, w1)     # the input is not written
        kernel_ms = ctx.cancel_timing()
        again = ctx.if_cancel(dev, plan.chans, plan.series, plan.amp, ms_done=plan.ms_done)
        try:
            assert again.clipped == total
            for (w0, w1), y in zip(plan.windows, got):
                assert again.download(w0, w1 - w0).tobytes() == y.tobytes(), (w0, w1)
        finally:
            again.free()
    finally:
        out.free()
    _report(capsys, "if_cancel over 2^32 + %d samples: %d windows under the rule (%d rounding decisions excluded), 2 untouched "
            "windows byte for byte, %d clipped exact, kernel %.1f ms" % (big.EXTRA32, len(got), sum(excluded), total, kernel_ms))


# ---- the probe and the monitor ------------------------------------------------------------------------------------------

def test_probe_stats_beyond_the_boundary(env, scene8, capsys):
    """10 code periods that start past 2^32 and 10 that straddle it, against the oracle on the downloaded window (which
    test_the_device_generator_beyond_the_boundaries ties to the host generator)."""
    m, s, ctx = env
    sc, dev, at = scene8
    worst = 0.0
    for w0, w1 in big.PROBE_WINDOWS:
        big.wrap_visible(at, big.identity, (w0, w0 + big.PROBE_RULE))
        x = dev.download(w0, w1 - w0)
        f, pxx, hist, nseg = ctx.probe_stats(dev, w0, w1 - w0, FS_MHZ)
        fo, po, ho = orc.probe_stats(orc.OracleSettings(), x)
        assert nseg == (w1 - w0 - 1024) // 15360 and np.array_equal(hist, ho) and np.array_equal(f, fo)
        worst = max(worst, float(np.max(np.abs(pxx - po) / po)))
    _report(capsys, "probe_stats past and across 2^32: PSD error %.3g per bin (bar %.0e)" % (worst, PSD_TOL))
    assert worst < PSD_TOL


def _spectrum_error(got, want):
    return float(np.abs(got - want).max() / want.max())


def test_the_monitor_over_the_whole_record(env, tiled, capsys):
    """offset 0, n = 2^32 + N + tail, N = 16384, no overlap, S = 2^32 - exactly WF_MAX_SLICE: one full slice of 262 144
    segments and a kept slice of one."""
    m, s, ctx = env
    rec, dev = tiled
    N, tail = big.WF_SEGMENT, big.WF_TAIL
    assert waterfall_spec.MAX_SLICE == B
    big.wrap_visible(rec.at, big.identity, (B, B + N + tail))
    want = big.waterfall_whole(rec, N, tail, FS_MHZ)
    assert want["phases"] == 105
    got = ctx.waterfall(dev, 0, B + N + tail, FS_MHZ, N, 0, B)
    assert got.pxx.shape == (2, N // 2 + 1)
    assert np.array_equal(got.n_segments, want["n_segments"]) and m._native.waterfall_plan(B + N + tail, N, 0, B) == 2
    assert np.array_equal(got.moments, want["moments"]), (got.moments, want["moments"])
    assert np.array_equal(got.hist, want["hist"])
    errs = [_spectrum_error(got.pxx[j], want["pxx"][j]) for j in (0, 1)]
    _report(capsys, "waterfall, S = 2^32: integers exact; spectrum error %.3g (slice 0, mean of 262 144 segments), %.3g "
            "(slice 1) of the largest bin (bar %.0e)" % (errs[0], errs[1], PSD_TOL))
    assert max(errs) < PSD_TOL
    assert np.array_equal(got.hold, got.pxx.max(axis=0))


def test_the_monitor_on_odd_bytes_past_the_boundary(env, tiled, capsys):
    m, s, ctx = env
    rec, dev = tiled
    off, n, N = big.WF_SECOND
    x = big.wrap_visible(rec.at, big.identity, (off, off + n))
    want = waterfall_spec.waterfall(x, 0, n, FS_MHZ, N, 0, N)
    got = ctx.waterfall(dev, off, n, FS_MHZ, N, 0, N)
    for k in ("n_segments", "moments", "hist", "f"):
        assert np.array_equal(getattr(got, k), want[k]), k
    err = max(_spectrum_error(g, w) for g, w in zip(got.pxx, want["pxx"]))
    _report(capsys, "waterfall at offset 2^32 - 3: spectrum error %.3g of the largest bin (bar %.0e)" % (err, PSD_TOL))
    assert got.pxx.shape == (3, N // 2 + 1) and err < PSD_TOL


# ---- acquisition --------------------------------------------------------------------------------------------------------

def test_the_acquisition_entry_points_across_the_boundary(env, scene8, capsys):
    """sgx_acquire on 11 code periods that start one period and 7 samples before 2^32 against the oracle on the downloaded
    window; the same search queued (acquire_begin / acquire_end) and sharded without a communicator, bit for bit; the
    coherent search with T = 2 against its contract."""
    m, s, ctx = env
    sc, dev, at = scene8
    w0, w1 = big.ACQ_WINDOW
    assert w0 == B - SPC - 7 and w1 - w0 == 12 * SPC
    big.wrap_visible(at, big.identity, (w0, w0 + big.PROBE_RULE))
    x = dev.download(w0, w1 - w0)
    n = 11 * SPC
    got = ctx.acquire(dev, w0, n, np.arange(32))
    ref = orc.acquire(orc.OracleSettings(), x[:n])
    det = np.asarray(ref["carrFreq"]) != 0
    assert sorted(np.flatnonzero(det) + 1) == [1, 3, 7, 11, 14, 19, 22, 31]
    assert np.array_equal(got["codePhase"], ref["codePhase"]) and np.array_equal(got["carrFreq"], ref["carrFreq"])
    for k in ("freqBin", "fineIdx"):
        assert np.array_equal(np.asarray(got[k])[det], np.asarray(ref[k])[det]), k
    err = float(np.max(np.abs(got["peakMetric"] / ref["peakMetric"] - 1.0)))
    assert np.allclose(got["peakMetric"], ref["peakMetric"], rtol=1e-9, atol=0)
    ctx.acquire_begin(dev, w0, n, np.arange(32))
    queued = ctx.acquire_end(32)
    sharded = ctx.acquire_sharded(None, 0, 1, dev, w0, n, n_prn_total=32)
    for k in got:
        assert np.array_equal(queued[k], got[k]) and queued[k].dtype == got[k].dtype, k
        assert np.array_equal(sharded[k], got[k].astype(sharded[k].dtype)), k
    prns = [0, 2, 5, 30]                                                       # PRN 1, 3 and 31 of the scene, PRN 6 absent
    coh = ctx.acquire_coherent(dev, w0, 12 * SPC, prns, coherent_ms=2, n_windows=2)
    want = coherent_acq_spec.acquire(s, x, 2, 2, False, None, prn_indices=prns)
    assert list(want["carrFreq"][prns] > 0) == [True, True, False, True]
    for k in ("carrFreq", "codePhase", "freqBin", "fineIdx"):
        assert np.array_equal(np.asarray(coh[k]), want[k][prns]), (k, coh[k], want[k][prns])
    assert np.allclose(coh["peakMetric"], want["peakMetric"][prns], rtol=1e-9, atol=0)
    _report(capsys, "acquire across 2^32: indices and carrFreq exact, peakMetric %.3g (bar 1e-9); queued and sharded bit for "
            "bit; coherent T = 2 exact, peakMetric %.3g" % (err, float(np.max(np.abs(coh["peakMetric"] /
                                                                                      want["peakMetric"][prns] - 1.0)))))


# ---- tracking -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tracked(env, scene8):
    """The window around 2^32 on the host, its eight channels acquired ON THE WINDOW (so the code phases are right at 112 s),
    and the oracle's series on it: 80 blocks from 20 code periods before the boundary on."""
    m, s, ctx = env
    sc, dev, at = scene8
    w0, w1 = big.TRACK_WINDOW
    big.wrap_visible(at, big.identity, (w0, w0 + big.PROBE_RULE))
    host = dev.download(w0, w1 - w0)
    a = m.AcquisitionResult(s, device=0)
    a.acquire(m.DeviceSignal(dev, w0, 11 * SPC))
    a.preRun()
    rel = [(int(c.PRN), float(c.acquiredFreq), float(c.codePhase)) for c in a.channels]
    assert sorted(c[0] for c in rel) == [1, 3, 7, 11, 14, 19, 22, 31] and all(0 <= c[2] < SPC for c in rel)
    so = orc.OracleSettings(numberOfChannels=8, msToProcess=float(big.TRACK_MS))
    ch = dict(PRN=np.array([c[0] for c in rel]), acquiredFreq=np.array([c[1] for c in rel]),
              codePhase=np.array([c[2] for c in rel]), status=['T'] * 8)
    want = orc.stack_series(orc.track(so, ch, host))
    want[:, 0] += w0                                           # (tests/test_big_record_host.py: the oracle does not care)
    assert np.all(want[:, 0, 0] < B) and np.all(want[:, 0, -1] > B + 50 * SPC)
    # one block of every channel straddles the boundary
    assert all(np.any((np.r_[w0 + rel[c][2], want[c, 0, :-1]] < B) & (want[c, 0] > B)) for c in range(8))
    absolute = [(p, f, w0 + cp) for p, f, cp in rel]
    return host, rel, absolute, want


def _same_as_the_oracle(capsys, what, got, done, want, tol=TRK_TOL):
    assert np.all(done == want.shape[2])
    assert np.array_equal(got[:, 0], want[:, 0]), what                        # absoluteSample: record positions past 2^32
    err = _trk_err(got, want)
    _report(capsys, "%s: absoluteSample exact, sums %.3g of RMS|P| (bar %.0e)" % (what, err, tol))
    assert err < tol, what


def test_track_int8_headline_kernel(env, scene8, tracked, capsys):
    """trk3_kernel through ctx.track.  The bar of tests/test_gpu_parity.py::test_random_scenes_against_oracle (the same
    kernel and sample type at position 0): absoluteSample exact, sums to 1e-6."""
    m, s, ctx = env
    host, rel, absolute, want = tracked
    got, done = ctx.track(scene8[1], absolute, big.TRACK_MS)
    tm = ctx.timing()
    assert tm["track_kernel"] == 5
    _same_as_the_oracle(capsys, "trk3_kernel, 8 channels across 2^32", got, done, want)


def _settings_at(m, skip):
    s = m.Settings()
    s.skipNumberOfBytes = int(skip)
    s.msToProcess = float(big.TRACK_MS)
    return s


def test_track_int8_through_the_drop_in_classes_and_the_queued_step(env, scene8, tracked, capsys):
    """Settings.skipNumberOfBytes near 2^32: acquire -> preRun -> track(DeviceFile) eagerly against the oracle (the bar of
    test_random_scenes_against_oracle), then the same queued - acquire_begin, the device-side preRun, the chained launch -
    bit for bit the eager run (tests/test_gpu_parity.py::test_deferred_step_equals_the_eager_one)."""
    m, s0, ctx0 = env
    host, rel, absolute, want = tracked
    dev = scene8[1]
    w0 = big.TRACK_WINDOW[0]
    runs = []
    for deferred in (False, True):
        s = _settings_at(m, w0)
        a = m.AcquisitionResult(s, device=0, deferred=deferred)
        a.acquire(m.DeviceSignal(dev, w0, 11 * SPC))
        a.preRun()
        t = m.TrackingResult(a, device=0)
        fid = m.DeviceFile(dev)
        t.track(fid)
        assert t.chained == deferred and m.engine.get_context(s, 0).timing()["track_kernel"] == 5
        runs.append((a, t, fid))
    (ae, te, fe), (ad, td, fd) = runs
    assert [(int(c.PRN), float(c.acquiredFreq), float(c.codePhase)) for c in ae.channels] == rel
    _same_as_the_oracle(capsys, "drop-in classes, skipNumberOfBytes = 2^32 - 20 code periods", te.series,
                        np.full(8, big.TRACK_MS), want)
    assert np.array_equal(td.series, te.series) and fd.tell() == fe.tell() == int(want[-1, 0, -1])
    for f in ("PRN", "acquiredFreq", "codePhase", "status"):
        assert np.array_equal(ad.channels[f], ae.channels[f]), f
    for f in ("carrFreq", "codePhase", "peakMetric"):
        assert np.array_equal(ad.results[f], ae.results[f]), f
    _report(capsys, "queued step (acquire_begin, device-side preRun, chained launch) across 2^32: bit for bit the eager run")


@pytest.mark.parametrize("var,value,members", [("SGX_TRK_V3", "0", 30), ("SGX_TRK_SPLIT", "1", 1)])
def test_track_int8_latency_kernel(env, scene8, tracked, capsys, var, value, members):
    """trk2_kernel (SGX_TRK_V3=0) and one workgroup per channel (SGX_TRK_SPLIT=1).  The bar of
    tests/test_gpu_parity.py::test_non_default_loop_and_search_settings, which runs these layouts against the oracle."""
    m, s, ctx = env
    host, rel, absolute, want = tracked
    old = os.environ.get(var)
    os.environ[var] = value
    try:
        got, done = ctx.track(scene8[1], absolute, big.TRACK_MS)
    finally:
        os.environ.pop(var, None) if old is None else os.environ.__setitem__(var, old)
    tm = ctx.timing()
    assert tm["track_kernel"] == 2 and tm["track_members"] == members
    _same_as_the_oracle(capsys, "trk2_kernel, %s=%s" % (var, value), got, done, want)


def test_track_int8_throughput_kernel(env, scene8, tracked, capsys):
    """trk_kernel_tp: 136 channels, the 8 inits replicated.  The bar of
    tests/test_gpu_parity.py::test_many_channels_at_staggered_offsets_against_the_oracle: sums to 1e-9, rates 1e-6 / 1e-5."""
    m, s, ctx = env
    host, rel, absolute, want = tracked
    got, done = ctx.track(scene8[1], [absolute[i % 8] for i in range(136)], big.TRACK_MS)
    tm = ctx.timing()
    assert tm["track_kernel"] == 3 and tm["track_members"] == 1
    for i in range(8, 136):
        assert np.array_equal(got[i], got[i % 8]), i
    _same_as_the_oracle(capsys, "trk_kernel_tp, 136 channels", got[:8], done[:8], want, 1e-9)
    assert np.max(np.abs(got[:8, 1] - want[:, 1])) < 1e-6 and np.max(np.abs(got[:8, 2] - want[:, 2])) < 1e-5


def test_replay_of_the_channels_tracked_across_the_boundary(env, scene8, tracked, capsys):
    """track_replay with a 5-tap bank over the blocks the headline kernel tracked, against replay_spec on the window: the bar
    of tests/test_replay_gpu.py::test_bank_of_21_taps_against_the_contract.  The states' `start` lies past 2^32."""
    m, s, ctx = env
    host, rel, absolute, want = tracked
    series, done = ctx.track(scene8[1], absolute, big.TRACK_MS)
    taps = (-1.0, -0.5, 0.0, 0.37, 1.5)
    got = ctx.track_replay(scene8[1], absolute, series, taps)
    state = m._native.replay_state(s, absolute, series, rec_bytes=len(scene8[1]))
    assert np.array_equal(state["start"][:, 1:], series[:, 0, :-1].astype(np.int64)) and np.all(state["start"][:, -1] > B)
    assert np.array_equal(state["start"][:, 0], np.array([int(c[2]) for c in absolute]))
    local = np.array(series)
    local[:, 0] -= big.TRACK_WINDOW[0]
    ref, _ = replay_spec.replay_channels(s, host, "int8", rel, local, None, taps)
    worst = 0.0
    for c in range(8):
        worst = max(worst, float(np.max(np.abs(got[c] - ref[c]))) / max(1.0, float(np.sqrt(np.mean(series[c, 3] ** 2
                                                                                                   + series[c, 7] ** 2)))))
    _report(capsys, "track_replay, 8 channels x 80 blocks x 5 taps across 2^32: %.3g of RMS|P| (bar %.0e)" % (worst, TRK_TOL))
    assert worst < TRK_TOL


def _sparse(ctx, n, start, payload, fill=0):
    """A record of n bytes of filler with the payload's bytes from `start` on, in HBM; the host array is let go at once."""
    raw = np.ascontiguousarray(payload).view(np.int8).ravel()
    b = np.zeros(n, dtype=np.int8) if fill == 0 else np.full(n, fill, dtype=np.uint8).view(np.int8)
    b[start:start + raw.size] = raw
    dev = ctx.upload(b)
    del b
    return dev


def _typed_case(m, ctx, capsys, what, payload, isz, rel, odd, data_type, dtype_name, kernel=None, fs=None, IF=None, fill=0):
    """payload: the window's samples in their type; the record is filler up to 2^32 - 20 code periods (in samples of the
    type) and the payload behind it, so that byte 2^32 lies inside the run.  rel: (prn, freq, sample phase) in the window;
    odd: channels (indices) started one byte late.  Against the oracle on the payload."""
    start = big.typed_start(isz, big.LOW_SPC if fs else SPC)
    raw = np.ascontiguousarray(payload).view(np.int8).ravel()
    n = start + raw.size
    at = big.sparse_reader(n, start, raw, fill)
    big.wrap_visible(at, big.identity, (start, start + big.PROBE_RULE), sparse=True)
    phase = [float(int(cp) * isz + (1 if i in odd else 0)) for i, (p, f, cp) in enumerate(rel)]
    so = orc.OracleSettings(numberOfChannels=len(rel), msToProcess=float(big.TRACK_MS), dataType=dtype_name, skipNumberOfBytes=0)
    if fs:
        so.samplingFreq, so.IF = fs, IF
    ch = dict(PRN=np.array([c[0] for c in rel]), acquiredFreq=np.array([c[1] for c in rel]), codePhase=np.array(phase),
              status=['T'] * len(rel))
    want = orc.stack_series(orc.track(so, ch, payload))
    want[:, 0] += start
    assert np.all(want[:, 0, 0] < B) and np.all(want[:, 0, -1] > B)
    dev = _sparse(ctx, n, start, raw, fill)
    try:
        got, done = ctx.track(dev, [(c[0], c[1], start + ph) for c, ph in zip(rel, phase)], big.TRACK_MS, data_type=data_type)
        tm = ctx.timing()
    finally:
        dev.free()
    if kernel is not None:
        assert tm["track_kernel"] == kernel, tm
    _same_as_the_oracle(capsys, "%s (kernel %d)" % (what, tm["track_kernel"]), got, done, want)


def test_track_int16_sparse_record(env, tracked, capsys):
    """The scene x 64 as int16 in the last window of 2^32 + window bytes of zeros: byte 2^32 is sample 2^31; the last channel
    starts on an odd byte.  The bar of tests/test_gpu_parity.py::test_track_int16_odd_start_byte_and_short_record."""
    m, s, ctx = env
    host, rel, absolute, want = tracked
    _typed_case(m, ctx, capsys, "int16 sparse record across byte 2^32", (host.astype(np.int16) * 64).astype("<i2"), 2,
                rel[:3], (2,), m._native.DT_INT16, "int16")


def test_track_float32_sparse_record(env, tracked, capsys):
    """float32 values in range: byte 2^32 is sample 2^30.  The bar of
    tests/test_gpu_parity.py::test_track_float32_record_matches_reference."""
    m, s, ctx = env
    host, rel, absolute, want = tracked
    payload = ((host.astype(np.int32) * 200 + 7) / 32768.0).astype("<f4")
    _typed_case(m, ctx, capsys, "float32 sparse record across byte 2^32", payload, 4, rel[:2], (), m._native.DT_FLOAT32,
                "float32")


LOW_FS, LOW_IF = big.LOW_FS, big.LOW_IF


def _low_rate(m):
    s = m.Settings()
    s.samplingFreq, s.IF = LOW_FS, LOW_IF
    n = s.samplesPerCode
    assert n == big.LOW_SPC
    sc = m.synth.Scene.make(*big.LOW_SCENE)
    os_ = orc.OracleSettings()
    os_.samplingFreq, os_.IF, os_.acqSatelliteList = LOW_FS, LOW_IF, range(1, 7)
    return s, sc, os_, n


def _low_rate_channels(os_, window, n):
    ch = orc.pre_run(os_, orc.acquire(os_, window[:11 * n]))
    rel = [(int(p), float(f), float(cp)) for p, f, cp in zip(ch["PRN"], ch["acquiredFreq"], ch["codePhase"]) if p]
    assert sorted(c[0] for c in rel) == [2, 5]
    return rel


def test_track_low_rate_int8_record_made_on_the_device(capsys):
    """trk_kernel_multi: a 4.092 Msps scene of 2^32 + 100 code periods made on the device at that rate.  The bar of
    tests/test_gpu_parity.py::test_other_front_ends_against_oracle[4092000.0-1023000.0]."""
    m = pkg()
    s, sc, os_, n = _low_rate(m)
    ctx = m.engine.get_context(s, 0)
    w0, w1 = big.low_rate_window()
    dev = ctx.synth(sc, big.LOW_N)
    try:
        host = dev.download(w0, w1 - w0)
        big.wrap_visible(big.scene_reader(m.synth.generate, sc), big.identity, (w0, w0 + big.PROBE_RULE))
        assert host[:50000].tobytes() == m.synth.generate(sc, 50000, offset=w0).tobytes()
        rel = _low_rate_channels(os_, host, n)
        so = orc.OracleSettings(numberOfChannels=2, msToProcess=float(big.TRACK_MS))
        so.samplingFreq, so.IF = LOW_FS, LOW_IF
        ch = dict(PRN=np.array([c[0] for c in rel]), acquiredFreq=np.array([c[1] for c in rel]),
                  codePhase=np.array([c[2] for c in rel]), status=['T'] * 2)
        want = orc.stack_series(orc.track(so, ch, host))
        want[:, 0] += w0
        got, done = ctx.track(dev, [(p, f, w0 + cp) for p, f, cp in rel], big.TRACK_MS)
        assert ctx.timing()["track_kernel"] == 4
        # the coherent kernel on the same device record and the same downloaded window (big.LOW_COHERENT: the boundary falls
        # in the pull-in, every group lies at 33-bit positions); the scene has no data bits, so any edge is a true one
        coh = big.LOW_COHERENT
        c0, c1 = big.low_rate_coherent_window()
        big.wrap_visible(big.scene_reader(m.synth.generate, sc), big.identity, (c0, c0 + big.PROBE_RULE))
        want_coh = coh_spec.track(so, rel, host, big.TRACK_MS, coh["T"], coh["P"], coh["H"], list(coh["edges"]))
        assert list(want_coh["ms_done"]) == [big.TRACK_MS] * 2 and list(want_coh["k0"]) == [43, 51]
        assert np.all(want_coh["series"][:, 0, 0] + w0 < big.B32) and np.all(want_coh["series"][:, 0, coh["P"] - 1] + w0 > big.B32)
        want_coh["series"][:, 0] += w0
        got_coh = ctx.track_coherent(dev, [(p, f, w0 + cp) for p, f, cp in rel], big.TRACK_MS,
                                     m._native.coh_params(s, coh["T"], coh["P"], coh["H"]), bit_edge=list(coh["edges"]))
        assert ctx.timing()["track_kernel"] == 7
    finally:
        dev.free()
    _same_as_the_oracle(capsys, "trk_kernel_multi at 4.092 Msps across 2^32", got, done, want)
    with capsys.disabled():
        _same_as_the_contract(got_coh, want_coh)


def test_track_low_rate_uint8_sparse_record(capsys):
    """trk_kernel_any: a sparse uint8 record at the same low rate, filled with 128.  The bar of
    tests/test_gpu_parity.py::test_track_low_rate_int16_and_uint8_against_the_oracle."""
    m = pkg()
    s, sc, os_, n = _low_rate(m)
    ctx = m.engine.get_context(s, 0)
    rec8 = m.synth.generate(sc, (big.TRACK_MS + 13) * n)
    rel = _low_rate_channels(os_, rec8, n)
    payload = (rec8.astype(np.int16) + 128).astype(np.uint8)
    _typed_case(m, ctx, capsys, "uint8 sparse record at 4.092 Msps across 2^32", payload, 1, rel, (), m._native.DT_UINT8,
                "uint8", kernel=6, fs=LOW_FS, IF=LOW_IF, fill=128)
