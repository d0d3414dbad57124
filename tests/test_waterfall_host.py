"""The record monitor without a GPU: the numpy contract of tests/waterfall_spec.py against independent ground - scipy's welch
per slice, the reference's own probeData spectrum, np.histogram and Python's big integers - then sgx_waterfall_plan against
the contract's slice counts, the event merging and the pulsed rule of frontend.py on hand-built arrays, every refusal, and
the false-alarm condition: the max-hold of the default scene without an interferer gives notch_design no line; and the
kernels' own work items in a host loop (sgx_waterfall_host) against the contract on every case and, at the probe's
parameters, against the oracle's probeData spectrum per bin.
Run with -m "not gpu"."""
import ctypes
import importlib

import numpy as np
import pytest

try:
    import scipy.signal
except ImportError:              # the restatement below stands in
    scipy = None

import waterfall_cases as cases
import waterfall_spec as spec
from conftest import load_golden, pkg, scene_from_json
from oracle import softgnss_oracle as orc

PSD_TOL = 1e-9     # tests/test_gpu_parity.py: relative, per bin


@pytest.fixture(scope="module")
def built():
    importlib.import_module("__graft_entry__").build()
    return pkg()


def welch(xs, fs, N, noverlap):
    """scipy's welch(xs, fs, hamming(N, periodic), N, noverlap, N, constant detrend, density, one-sided); without scipy a
    direct restatement written apart from the contract: float detrend, np.hamming's formula, the mean over a 2-D rfft."""
    if scipy is not None:
        return scipy.signal.welch(xs, fs, scipy.signal.get_window("hamming", N, fftbins=True), N, noverlap, N,
                                  detrend="constant", scaling="density", return_onesided=True)
    step = N - noverlap
    starts = np.arange(0, xs.size - N + 1, step)
    segs = np.stack([xs[a:a + N] for a in starts])
    segs = segs - segs.mean(axis=1, keepdims=True)
    win = np.hamming(N + 1)[:N]
    p = np.abs(np.fft.rfft(segs * win, axis=1)) ** 2 / (fs * (win ** 2).sum())
    p[:, 1:N // 2] *= 2.0
    return np.fft.rfftfreq(N, 1.0 / fs), p.mean(axis=0)


# the records the independent checks run on: the big ones only cost time and add no shape
SMALL = [c for c in cases.CASES if c.n <= 200000]


@pytest.mark.parametrize("c", SMALL, ids=[c.name for c in SMALL])
def test_the_contract_is_scipy_s_welch_per_slice(c):
    want = cases.want(c)
    x = cases.record(c)[c.offset:c.offset + c.n]
    assert len(want["n_segments"]) == len(spec.plan(c.n, c.N, c.noverlap, c.S))
    for j, (start, length, K) in enumerate(spec.plan(c.n, c.N, c.noverlap, c.S)):
        xs = x[start:start + length].astype(np.float64)
        f, pxx = welch(xs, cases.FS_MHZ, c.N, c.noverlap)
        assert want["n_segments"][j] == K == (length - c.noverlap) // (c.N - c.noverlap)
        assert np.allclose(f, want["f"], rtol=1e-15, atol=0)
        top = pxx.max()
        if c.content in ("min", "max", "const") or not xs.any():
            assert not want["pxx"][j].any()                      # exactly zero; a float detrend may leave rounding
            assert top < 1e-20
        else:
            assert np.abs(want["pxx"][j] - pxx).max() / top < PSD_TOL
    assert np.array_equal(want["hold"], want["pxx"].max(axis=0))


def test_slice_0_at_the_probe_s_parameters_is_the_reference_s_spectrum():
    g = load_golden("probe_default.npz")
    n = int(g["n_samples"])
    data = pkg("synth").generate(scene_from_json(g["scene"]), n)
    w = spec.waterfall(data, 0, n, 38.192, 16384, 1024, n)
    assert w["pxx"].shape == (1, 8193) and int(w["n_segments"][0]) == 24
    assert np.array_equal(w["f"], g["f"])
    assert np.max(np.abs(w["pxx"][0] - g["Pxx"]) / g["Pxx"]) < PSD_TOL
    assert np.array_equal(w["hist"][0, :254], g["hist"][:254]) and w["hist"][0, 254:].sum() == g["hist"][254]


@pytest.mark.parametrize("c", cases.CASES, ids=[c.name for c in cases.CASES])
def test_the_integers_against_histogram_and_big_integers(c):
    want = cases.want(c)
    x = cases.record(c)[c.offset:c.offset + c.n]
    rows = range(len(want["n_segments"])) if c.n <= 200000 else (0, len(want["n_segments"]) - 1)
    for j in rows:
        start, length, _ = spec.plan(c.n, c.N, c.noverlap, c.S)[j]
        vals = [int(v) for v in x[start:start + length]]
        assert [int(v) for v in want["moments"][j]] == [len(vals), sum(vals), sum(v * v for v in vals),
                                                        sum(v ** 4 for v in vals)]
        assert np.array_equal(want["hist"][j], np.histogram(x[start:start + length], bins=256, range=(-128.5, 127.5))[0])
    assert int(want["moments"][:, 0].sum()) == sum(p[1] for p in spec.plan(c.n, c.N, c.noverlap, c.S))


def test_the_extremes_fit_int64():
    assert spec.MAX_SLICE * 128 ** 4 < 2 ** 63               # the longest slice, every sample on -128
    m, h = spec.slice_stats(np.full(1000, -128, dtype=np.int8))
    assert [int(v) for v in m] == [1000, -128000, 1000 * 128 ** 2, 1000 * 128 ** 4] and h[0] == 1000 and h[1:].sum() == 0


def test_derived_figures(built):
    rng = np.random.default_rng(3)
    x = np.clip(np.rint(rng.normal(2.0, 30.0, 40000)), -128, 127).astype(np.int8)
    x[:50] = -128
    m, h = spec.slice_stats(x)
    mean, rms, kurt, clip = spec.derived(m[None], h[None])
    v = x.astype(np.float64)
    d = v - v.mean()
    assert np.isclose(mean[0], v.mean(), rtol=1e-13) and np.isclose(rms[0], np.sqrt((v * v).mean()), rtol=1e-13)
    assert np.isclose(kurt[0], (d ** 4).mean() / (d * d).mean() ** 2 - 3.0, rtol=1e-10)
    assert clip[0] == ((x == -128) | (x == -127) | (x == 127)).sum() / x.size
    w = built._native.Waterfall(np.zeros(1), np.zeros((1, 1)), np.zeros(1), m[None], h[None], np.ones(1, dtype=np.int64), 40000)
    assert (w.mean[0], w.rms[0], w.kurtosis[0], w.clip_share[0]) == (mean[0], rms[0], kurt[0], clip[0])
    const = spec.derived(*[a[None] for a in spec.slice_stats(np.full(100, 5, dtype=np.int8))])
    assert const[0][0] == 5.0 and const[1][0] == 5.0 and const[2][0] == 0.0 and const[3][0] == 0.0


@pytest.mark.parametrize("c", cases.CASES, ids=[c.name for c in cases.CASES])
def test_the_library_s_plan_counts_the_contract_s_slices(built, c):
    assert built._native.waterfall_plan(c.n, c.N, c.noverlap, c.S) == len(spec.plan(c.n, c.N, c.noverlap, c.S))


def test_the_plan_on_lengths_around_every_boundary(built):
    for N, noverlap, S in ((256, 0, 256), (256, 255, 300), (1024, 64, 5000), (16384, 1024, 3819200)):
        for n in (N, N + 1, S - 1, S, S + 1, S + N - 1, S + N, 3 * S + N - 1, 3 * S + N, 7 * S):
            if n >= N:
                assert built._native.waterfall_plan(n, N, noverlap, S) == len(spec.plan(n, N, noverlap, S)), (N, noverlap, S, n)


REFUSED = [dict(n=5000, N=1000, noverlap=0, S=2048), dict(n=5000, N=128, noverlap=0, S=2048),
           dict(n=50000, N=32768, noverlap=0, S=32768), dict(n=5000, N=0, noverlap=0, S=2048),
           dict(n=5000, N=1024, noverlap=1024, S=2048), dict(n=5000, N=1024, noverlap=-1, S=2048),
           dict(n=5000, N=1024, noverlap=0, S=1023), dict(n=5000, N=1024, noverlap=0, S=2 ** 32 + 1),
           dict(n=1023, N=1024, noverlap=0, S=1024), dict(n=0, N=256, noverlap=0, S=256)]


@pytest.mark.parametrize("r", REFUSED, ids=["n%(n)d-N%(N)d-o%(noverlap)d-S%(S)d" % r for r in REFUSED])
def test_refusals(built, r):
    with pytest.raises(ValueError):
        spec.check(r["n"], r["N"], r["noverlap"], r["S"])
    with pytest.raises(ValueError):
        built._native.waterfall_plan(r["n"], r["N"], r["noverlap"], r["S"])
    rc = built._native.lib().sgx_waterfall_plan(r["n"], r["N"], r["noverlap"], r["S"], ctypes.byref(ctypes.c_int64(0)))
    short = r["n"] < r["N"] and 256 <= r["N"] <= 16384 and 0 <= r["noverlap"] < r["N"] and r["N"] <= r["S"] <= 2 ** 32
    assert rc == (built._native.SGX_E_RANGE if short else built._native.SGX_E_ARG)
    assert ("ValueError" in built._native.last_error()) == short


def test_notch_whole_record_needs_notch(built, monkeypatch, capsys):
    def never(self, *args, **kw):
        raise AssertionError("the run went on")

    for method in ("postProcessing", "probeData", "_prepared_record"):
        monkeypatch.setattr(built.Settings, method, never)
    for argv, word in ((["x.bin", "--notch-whole-record"], "--notch"), (["x.bin", "--monitor-out", "a.npz"], "--monitor"),
                       (["x.bin", "--monitor=0"], "--monitor"), (["x.bin", "--monitor=-5"], "--monitor")):
        with pytest.raises(SystemExit) as e:
            pkg("main").main(argv)
        assert e.value.code == 2
        captured = capsys.readouterr()
        assert word in captured.err.split(": error: ", 1)[1] and "Welcome" not in captured.out


def test_the_options_reach_the_settings(built, monkeypatch, capsys):
    seen = {}
    monkeypatch.setattr(built.Settings, "postProcessing",
                        lambda self, fileNameStr=None: seen.update(vars(self)) or (None, None, None))
    monkeypatch.setattr(pkg("main"), "monitor_file", lambda settings, out=None: seen.update(out=out, monitored=True))
    assert pkg("main").main(["x.bin", "--no-probe"]) == 0
    assert (seen["monitorSliceMs"], seen["monitorSegment"], seen["monitorOverlap"], seen["monitorMinSlices"],
            seen["notchWholeRecord"]) == (100.0, 16384, 1024, 2, False) and "monitored" not in seen
    assert pkg("main").main(["x.bin", "--no-probe", "--notch", "--notch-whole-record", "--monitor=50", "--monitor-out", "a.npz"]) == 0
    assert seen["notchWholeRecord"] is True and seen["interferenceMitigation"] is True and seen["monitorSliceMs"] == 50.0
    assert seen["monitored"] and seen["out"] == "a.npz"
    for option in ("--monitor", "--monitor-out", "--notch-whole-record"):
        assert option in pkg("main").__doc__


# ---- the kernels' work items in a host loop -------------------------------------------------------------------------------

@pytest.mark.parametrize("c", cases.CASES, ids=[c.name for c in cases.CASES])
def test_the_host_items_equal_the_contract(built, c):
    """Every segment length 256 .. 16384 and every step pattern of the transform (2.4.16^n, 16^n, 4.16^n, 2.16^n) without a
    GPU: the bar of tests/test_waterfall_gpu.py, PSD_TOL of the slice's largest bin; a slice that must be zero is +0.0."""
    want = cases.want(c)
    pxx, nseg = built._native.waterfall_host(cases.record(c)[c.offset:c.offset + c.n], cases.FS_MHZ, c.N, c.noverlap, c.S)
    assert pxx.shape == want["pxx"].shape and np.array_equal(nseg, want["n_segments"])
    worst = 0.0
    for g, w in zip(pxx, want["pxx"]):
        if w.max() == 0.0:
            assert not g.any() and not np.signbit(g).any()
        else:
            worst = max(worst, float(np.abs(g - w).max() / w.max()))
    print("%s: spectrum error %.3g of the slice's largest bin" % (c.name, worst))
    assert worst < PSD_TOL


def test_the_host_items_at_the_probe_s_parameters_are_the_oracle_s_probe_stats(built):
    """sgx_probe_stats is the monitor at N = 16384, overlap 1024, one slice: its arithmetic on the windows of
    tests/test_gpu_parity.py::test_probe_statistics_golden, held to the oracle per bin as that test holds the GPU."""
    rng = np.random.default_rng(21)
    x = rng.integers(-128, 128, size=500000, dtype=np.int8)
    x[1000:1200] = -128
    x[5000:5100] = 127
    s2 = orc.OracleSettings()
    s2.samplingFreq = 16367600.0
    for off, n in ((0, 381920), (12345, 300001), (7, 16384), (99, 16385 + 15359)):
        pxx, nseg = built._native.waterfall_host(x[off:off + n], 16.3676, 16384, 1024, n)
        fo, po, ho = orc.probe_stats(s2, x[off:off + n])
        assert pxx.shape == (1, 8193) and int(nseg[0]) == (n - 1024) // 15360
        worst = float(np.max(np.abs(pxx[0] - po) / po))
        print("window (%d, %d): PSD error %.3g per bin" % (off, n, worst))
        assert worst < PSD_TOL


# ---- events and pulsed slices ---------------------------------------------------------------------------------------------

def test_events_merge_across_consecutive_slices(built):
    fe = pkg("frontend")
    A, B = 9.728e6, 12.0e6
    per_slice = [
        [],
        [(A, 80e3, 20.0)],                                   # A: slices 1 .. 3, drifting by less than its width per slice
        [(A + 30e3, 80e3, 30.0), (B, 80e3, 12.0)],           # B: slice 2 only -> dropped at min_slices = 2
        [(A + 60e3, 100e3, 25.0)],
        [],
        [(A, 80e3, 15.0)],                                   # A again after a gap: a new event, slices 5 .. 6
        [(A, 80e3, 16.0), (A + 200e3, 80e3, 9.0)],           # a neighbour whose band does not overlap: its own, 1 slice
    ]
    for merge in (spec.merge_events, fe.monitor_events):
        got = merge(per_slice, 100.0, 2)
        assert got == [(A + 30e3, 100e3, 100.0, 400.0, 30.0), (A, 80e3, 500.0, 700.0, 16.0)]
        every = merge(per_slice, 100.0, 1)
        assert len(every) == 4 and (B, 80e3, 200.0, 300.0, 12.0) in every and (A + 200e3, 80e3, 600.0, 700.0, 9.0) in every
        assert merge([], 100.0, 2) == [] and merge([[], []], 100.0, 1) == []
    # a line that drifts further than its band per slice does not merge
    far = [[(A, 80e3, 10.0)], [(A + 81e3, 80e3, 10.0)]]
    assert fe.monitor_events(far, 100.0, 1) == spec.merge_events(far, 100.0, 1) and len(fe.monitor_events(far, 100.0, 1)) == 2


def test_the_pulsed_rule_reads_the_record_s_own_spread(built):
    fe = pkg("frontend")
    rng = np.random.default_rng(11)
    kurt = -0.15 + 0.002 * rng.standard_normal(200)
    clip = np.zeros(200)
    for rule in (spec.pulsed, fe.monitor_pulsed):
        assert rule(kurt, clip) == []
        k2, c2 = kurt.copy(), clip.copy()
        k2[17] = 0.4                                          # a burst of pulses: heavy tails in one slice
        c2[90] = 1e-4                                         # a slice that clips where no other does
        assert rule(k2, c2) == [17, 90]
        assert rule(k2 + 5.0, c2) == [17, 90]                 # a record that is heavy-tailed throughout: the same slices
        assert rule(50.0 * k2, c2) == [17, 90] and rule(np.zeros(0), np.zeros(0)) == []
        assert rule(np.full(10, 3.0), np.full(10, 0.25)) == []   # steady at any level: nothing stands out


def test_line_peak_db(built):
    fe = pkg("frontend")
    f = np.arange(8193) * (38.192 / 16384)
    pxx = np.full(8193, 2.0)
    pxx[4000] = 2000.0
    assert abs(fe.line_peak_db(f, pxx, f[4000] * 1e6, 80e3) - 30.0) < 1e-9


# ---- the false-alarm condition --------------------------------------------------------------------------------------------

@pytest.mark.slow
def test_the_clean_scene_gives_the_whole_record_notch_no_line(built):
    """2 s of the default scene without an interferer, the default monitor settings (100 ms slices, 16384 / 1024): the
    max-hold over 20 slices is the largest of 20 estimates per bin, each a mean of 248 segments - it must not cross the
    notch's 8 dB over the running median anywhere, or notchWholeRecord would filter a clean record."""
    s = built.Settings()
    assert (s.monitorSliceMs, s.monitorSegment, s.monitorOverlap, s.notchThresholdDb) == (100.0, 16384, 1024, 8.0)
    n = int(2.0 * s.samplingFreq)
    x = built.synth.generate(built.synth.Scene.default(), n)
    w = spec.waterfall(x, 0, n, s.samplingFreq / 1e6, int(s.monitorSegment), int(s.monitorOverlap),
                       int(np.rint(s.monitorSliceMs * 1e-3 * s.samplingFreq)))
    assert len(w["n_segments"]) == 20
    lines = built._native.notch_design(s, w["f"], w["hold"], s.notchThresholdDb, s.notchWidthHz, s.notchTaps)[2]
    assert lines == []
    assert pkg("frontend").monitor_pulsed(*spec.derived(w["moments"], w["hist"])[2:]) == []
