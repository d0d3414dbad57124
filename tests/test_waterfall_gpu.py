"""The record monitor on the GPU (sgx_probe_waterfall, csrc/sgx_waterfall.hip; Settings.monitorRecord, mitigate with
notchWholeRecord): the kernels against the numpy contract of tests/waterfall_spec.py on every case of tests/waterfall_cases.py -
the integers exactly, the spectra to the bar of the probeData parity test taken relative to the slice's largest bin - and
against the host run of the same work items (sgx_waterfall_host) bit for bit; then sgx_probe_stats, which is the monitor at
its own parameters, on the same window, a streaming record, and end to end a scene whose jammer switches on late."""
import tempfile

import numpy as np
import pytest

import notch_cases
import waterfall_cases as cases
from conftest import pkg

pytestmark = pytest.mark.gpu

# The bar of tests/test_gpu_parity.py's probeData parity (PSD_TOL: fp64 FFT with another operation order than pocketfft),
# here on the error relative to the slice's largest bin.  Measured over the whole table, GPU against contract: 2.2e-15 at the
# worst case, grid-8192-0, so no case needs more.
PSD_TOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    m = pkg()
    return m.engine.get_context(m.Settings(), 0)


def run(ctx, c, rec=None):
    own = rec is None
    if own:
        rec = ctx.upload(cases.record(c))
    try:
        return ctx.waterfall(rec, c.offset, c.n, cases.FS_MHZ, c.N, c.noverlap, c.S)
    finally:
        if own:
            rec.free()


def spectrum_error(got, want):
    """The largest error of a [slices][bins] spectrum relative to each slice's largest bin; a slice that must be all zero
    must be exactly that."""
    worst = 0.0
    for g, w in zip(np.atleast_2d(got), np.atleast_2d(want)):
        top = w.max()
        if top == 0.0:
            assert not g.any(), "a slice that must be exactly zero is not"
        else:
            worst = max(worst, float(np.abs(g - w).max() / top))
    return worst


@pytest.mark.parametrize("c", cases.CASES, ids=[c.name for c in cases.CASES])
def test_case_equals_the_contract(ctx, c):
    want = cases.want(c)
    got = run(ctx, c)
    assert got.pxx.shape == want["pxx"].shape
    assert np.array_equal(got.n_segments, want["n_segments"])
    assert np.array_equal(got.moments, want["moments"])
    assert np.array_equal(got.hist, want["hist"])
    assert np.array_equal(got.f, want["f"])
    err = max(spectrum_error(got.pxx, want["pxx"]), spectrum_error(got.hold, want["hold"]))
    print("%s: spectrum error %.3g of the slice's largest bin" % (c.name, err))
    assert err < PSD_TOL
    assert np.array_equal(got.hold, got.pxx.max(axis=0))


@pytest.mark.parametrize("c", cases.CASES, ids=[c.name for c in cases.CASES])
def test_case_equals_the_host_items_bit_for_bit(ctx, c):
    got = run(ctx, c)
    pxx, nseg = pkg()._native.waterfall_host(cases.record(c)[c.offset:c.offset + c.n], cases.FS_MHZ, c.N, c.noverlap, c.S)
    assert np.array_equal(got.n_segments, nseg)
    assert got.pxx.tobytes() == pxx.tobytes()
    assert got.hold.tobytes() == pxx.max(axis=0).tobytes()


@pytest.mark.parametrize("name", ["constant", "constant-16384", "all-min", "all-max"])
def test_a_constant_record_gives_exactly_zero(ctx, name):
    got = run(ctx, cases.BY_NAME[name])
    assert got.pxx.size and not got.pxx.any() and not got.hold.any()
    assert np.array_equal(np.signbit(got.pxx), np.zeros(got.pxx.shape, dtype=bool))      # 0.0, not -0.0


@pytest.mark.parametrize("name", ["alternating", "alternating-16384"])
def test_alternating_full_scale_puts_the_power_at_the_last_bin(ctx, name):
    got = run(ctx, cases.BY_NAME[name])
    assert np.all(got.pxx.argmax(axis=1) == got.pxx.shape[1] - 1)
    # the Hamming window spreads a line on a bin centre over that bin and its neighbours (0.54, 0.23, 0.23) and no further;
    # below bin N/2 - 1 rounding alone: an amplitude error of a few eps per pass, 64 eps at most, squared
    assert np.all(got.pxx[:, :-2].max(axis=1) < (64 * np.finfo(np.float64).eps) ** 2 * got.pxx[:, -1])


def test_the_late_tone_shows_in_the_second_half_only(ctx):
    c = cases.BY_NAME["late-tone"]
    got = run(ctx, c)
    half = len(got.n_segments) // 2
    assert not got.pxx[:half].any()
    assert np.all(got.pxx[half:].argmax(axis=1) == cases.TONE_BIN) and int(got.hold.argmax()) == cases.TONE_BIN


@pytest.mark.parametrize("name", ["grid-16384-1024", "chunk-cuts-slice", "many-slices"])
def test_two_calls_are_bit_identical(ctx, name):
    c = cases.BY_NAME[name]
    rec = ctx.upload(cases.record(c))
    a, b = run(ctx, c, rec), run(ctx, c, rec)
    rec.free()
    for k in ("pxx", "hold", "moments", "hist", "n_segments"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def test_slice_0_at_the_probe_s_parameters_is_probe_stats(ctx):
    """sgx_probe_stats is the monitor with one slice of the window at N = 16384, noverlap = 1024: the same bits."""
    n = 10 * 38192
    x = np.clip(np.rint(np.random.default_rng(5).normal(3.0, 12.0, n + 7)), -127, 127).astype(np.int8)
    rec = ctx.upload(x)
    f, pxx, hist, nseg = ctx.probe_stats(rec, 7, n, cases.FS_MHZ)
    got = ctx.waterfall(rec, 7, n, cases.FS_MHZ, 16384, 1024, n)
    rec.free()
    assert got.pxx.shape == (1, 8193) and int(got.n_segments[0]) == nseg == 24
    assert np.array_equal(got.f, f)
    assert np.array_equal(got.pxx[0], pxx)
    assert np.array_equal(got.hist[0, :254], hist[:254]) and got.hist[0, 254] + got.hist[0, 255] == hist[254]


def test_probe_stats_leaves_the_monitor_s_timing(ctx):
    c = cases.BY_NAME["grid-16384-1024"]
    rec = ctx.upload(cases.record(c))
    run(ctx, c, rec)
    before = ctx.waterfall_timing()
    ctx.probe_stats(rec, c.offset, c.n, cases.FS_MHZ)
    assert before > 0.0 and ctx.waterfall_timing() == before
    rec.free()


def test_a_streaming_record_gives_the_same_arrays(ctx):
    c = cases.BY_NAME["chunk-cuts-slice"]
    resident = run(ctx, c)
    with tempfile.NamedTemporaryFile(suffix=".bin") as fh:
        cases.record(c).tofile(fh.name)
        rec = ctx.open_file(fh.name, 0, cases.record(c).size)
        streamed = run(ctx, c, rec)
        rec.free()
    for k in ("pxx", "hold", "moments", "hist", "n_segments"):
        assert getattr(resident, k).tobytes() == getattr(streamed, k).tobytes(), k


def test_refusals_on_the_device(ctx):
    rec = ctx.upload(np.zeros(5000, dtype=np.int8))
    for args in ((0, 5000, 1000, 0, 2048), (0, 5000, 32768, 0, 32768), (0, 5000, 1024, 1024, 2048), (0, 5000, 1024, -1, 2048),
                 (0, 5000, 1024, 0, 1023), (0, 1023, 1024, 0, 1024), (4000, 2000, 1024, 0, 1024)):
        with pytest.raises(ValueError):
            ctx.waterfall(rec, args[0], args[1], cases.FS_MHZ, args[2], args[3], args[4])
    rec.free()


def test_a_jammer_that_switches_on_late_is_seen_and_notched():
    """0.5 s of the default scene, a 100-LSB line at IF + 180 kHz from 0.25 s on: the spectrum of the first 10 ms shows no
    line; the monitor's max-hold does, and dates it."""
    m = pkg()
    s = m.Settings()
    c = m.engine.get_context(s, 0)
    n = int(0.5 * s.samplingFreq)
    clean = c.synth(m.synth.Scene.default(), n)
    x = clean.download()
    clean.free()
    half = n // 2
    x[half:] = notch_cases.jam(x, s.samplingFreq, s.IF + notch_cases.CW_OFFSET_HZ)[half:]
    rec = c.upload(x)
    same, lines = s.mitigate(rec)
    assert lines == [] and same is rec
    s.notchWholeRecord = True
    new, lines = s.mitigate(rec)
    assert len(lines) == 1 and abs(lines[0][0] - (s.IF + notch_cases.CW_OFFSET_HZ)) <= s.notchWidthHz
    assert new is not rec and len(new) == len(rec)
    events = s.lastMonitor["events"]
    assert len(events) == 1
    f_hz, width_hz, first_ms, last_ms, peak_db = events[0]
    assert abs(f_hz - (s.IF + notch_cases.CW_OFFSET_HZ)) <= s.notchWidthHz
    assert abs(first_ms - 250.0) <= s.monitorSliceMs and last_ms == 500.0 and peak_db > s.notchThresholdDb
    assert s.lastMonitor["pulsed"] == []
    new.free()
    rec.free()


def test_the_command_line_monitors_prints_and_saves(monkeypatch, capsys, tmp_path):
    """--monitor=10 on a 100 ms file whose line comes up at 50 ms: a line per event, the arrays in the .npz; --notch with
    --notch-whole-record then reaches postProcessing, which is stubbed here - acquisition and tracking are not the point."""
    m = pkg()
    s = m.Settings()
    c = m.engine.get_context(s, 0)
    n = 100 * s.samplesPerCode
    clean = c.synth(m.synth.Scene.default(), n)
    x = clean.download()
    clean.free()
    x[n // 2:] = notch_cases.jam(x, s.samplingFreq, s.IF + notch_cases.CW_OFFSET_HZ)[n // 2:]
    path, out = str(tmp_path / "late.bin"), str(tmp_path / "seen.npz")
    x.tofile(path)
    seen = {}
    monkeypatch.setattr(m.Settings, "postProcessing", lambda self, fileNameStr=None: seen.update(vars(self)) or (None,) * 3)
    assert pkg("main").main([path, "--no-probe", "--ms", "98", "--monitor=10", "--monitor-out", out, "--notch",
                             "--notch-whole-record"]) == 0
    printed = capsys.readouterr().out
    assert "10 slices of 10.0 ms, 24 Welch segments each" in printed
    assert "Line at 9.72" in printed and "from 50 to 100 ms" in printed and "Nothing stands out" not in printed
    assert seen["notchWholeRecord"] is True and seen["monitorSliceMs"] == 10.0
    info = seen["lastMonitor"]
    assert len(info["events"]) == 1 and info["events"][0][2:4] == (50.0, 100.0)
    saved = np.load(out)
    assert saved["pxx"].shape == (10, 8193) and saved["events"].shape == (1, 5) and saved["hist"].shape == (10, 256)
    assert np.array_equal(saved["pxx"], info["waterfall"].pxx) and int(saved["moments"][:, 0].sum()) == n
    # ... and the prepared record postProcessing would read: notched from the monitor's max-hold, the event printed
    s2 = m.Settings()
    s2.notchWholeRecord, s2.monitorSliceMs = True, 10.0
    with s2._prepared_record(path, 0, n, mitigate_at=0, verbose=True) as rec:
        assert len(rec) == n
    printed = capsys.readouterr().out
    assert "Removed a line at 9.72" in printed and "Seen from 50 to 100 ms: a line at 9.72" in printed
    assert len(s2.lastNotchLines) == 1 and s2.lastMonitor["events"][0][2:4] == (50.0, 100.0)
    s2.notchWholeRecord = False                              # as before: the first 10 ms show nothing
    with s2._prepared_record(path, 0, n, mitigate_at=0, verbose=True) as rec:
        assert len(rec) == n
    assert "No narrowband interference found" in capsys.readouterr().out and s2.lastNotchLines == []
