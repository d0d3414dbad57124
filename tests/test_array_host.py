"""CPU-only checks of the multi-antenna combiner (include/sgx.h: sgx_array_design, and what of the stage needs no record)
against the numpy contract of tests/array_spec.py: the design to the bit and against an independent solver, its refusals,
the scenes of tests/array_cases.py shown to be what they claim by the contracts plus the oracle alone - no single antenna
acquires, the combined record does -, the Settings surface with its walk and its refusals, the unpacker's selection with
antennas, and the command line through a stubbed postProcessing.  Run with -m "not gpu"."""
import ctypes as C
import importlib

import numpy as np
import pytest

import array_cases as cases
import array_spec as spec
from conftest import pkg

SHAPES = [(A, K) for A in (2, 3, 4, 8) for K in (1, 3, 7, 15) if A * K <= spec.MAX_WEIGHTS]


@pytest.fixture(scope="module")
def built():
    importlib.import_module("__graft_entry__").build()
    return pkg()


def correlated_record(rng, frames, lanes, A):
    """Streams that share two sources of their own colour under noise of their own: statistics that are Hermitian and
    positive definite, with off-diagonal terms at every lag."""
    src = rng.standard_normal((2, frames + 4, lanes)) * 25.0
    src = src[:, 4:] + 0.6 * src[:, 2:-2] - 0.3 * src[:, :-4]
    mix = rng.uniform(-1.0, 1.0, (A, 2))
    x = np.einsum("as,sfl->fal", mix, src) + 6.0 * rng.standard_normal((frames, A, lanes))
    if lanes == 2:                             # a rotation per antenna and source: complex cross terms
        x[:, :, 1] += np.einsum("as,sf->fa", rng.uniform(-1.0, 1.0, (A, 2)), src[:, :, 0])
    return np.clip(np.rint(x), -128, 127).astype(np.int8).reshape(-1)


def same_design(n, rho, frames, lanes, ref, loading=spec.DEFAULT_LOADING, target=spec.DEFAULT_TARGET_RMS):
    want = spec.design(rho, frames, lanes, ref, loading, target)
    taps, shift, info = n.array_design(rho, frames, lanes, ref, loading, target)
    assert taps.dtype == np.int16 and taps.shape == want[0].shape and np.array_equal(taps, want[0])
    assert shift == want[1] == spec.DESIGN_SHIFT == n.ARRAY_SHIFT
    assert info["gain"] == want[2] and info["suppression_db"] == want[3]       # exactly
    assert np.array_equal(info["weights"], want[4])
    spec.check(taps, shift, lanes, rho.shape[0])                               # what it designs, the combiner takes
    return want


def solved_weights(rho, frames, lanes, ref, loading):
    """The weights by numpy.linalg.solve of the same loaded system, complex where the record is."""
    P, Q = spec.covariance(rho, frames, lanes)
    R = np.array(P) + 1j * np.array(Q)
    n = R.shape[0]
    K = rho.shape[2]
    RL = R + loading * np.trace(R).real / n * np.eye(n)
    e = np.zeros(n)
    e[ref * K + (K - 1) // 2] = 1.0
    g = np.linalg.solve(RL, e)
    g = g / g[ref * K + (K - 1) // 2].real
    return np.conj(g).reshape(rho.shape[0], K)


# ---- the design function ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("A,K", SHAPES)
def test_design_equals_the_contract(built, lanes, A, K):
    n = built._native
    rng = np.random.default_rng(100 * A + 10 * K + lanes)
    frames = 3000
    rho = spec.stats(correlated_record(rng, frames, lanes, A), lanes, A, K)
    assert np.array_equal(rho[:, :, 0, 0], rho[:, :, 0, 0].T)                  # Hermitian at lag 0
    for ref, loading, target in ((0, spec.DEFAULT_LOADING, 12.0), (A - 1, 0.0, 5.5), (A // 2, 0.05, 20.0)):
        want = same_design(n, rho, frames, lanes, ref, loading, target)
        w = solved_weights(rho, frames, lanes, ref, loading)
        assert np.max(np.abs(want[4] - (w if lanes == 2 else w.real))) <= 1e-9 * np.max(np.abs(w))
        if lanes == 1:
            assert np.max(np.abs(w.imag)) == 0.0
        c = (K - 1) // 2
        assert abs(want[4][ref, c] - 1.0) < 1e-12 and want[3] >= -1e-9        # the constraint holds; never worse than ref alone


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_design_of_the_scenes(built, name):
    scene = cases.SCENES[name]
    frames = cases.ACQ_MS * scene.frames_per_ms
    c = cases.combined(scene, frames)
    want = same_design(built._native, c["rho"], frames, scene.lanes, 0)
    assert want[3] == c["suppression_db"] and np.array_equal(want[0], c["taps"])
    w = solved_weights(c["rho"], frames, scene.lanes, 0, spec.DEFAULT_LOADING)
    assert np.max(np.abs(c["weights"] - (w if scene.lanes == 2 else w.real))) <= 1e-9 * np.max(np.abs(w))
    assert np.allclose(spec.input_rms(c["rho"], frames), np.sqrt(cases.JAMMER_SIGMA ** 2 + cases.NOISE_SIGMA ** 2), rtol=0.02)


def _design_rc(n, rho, frames=1000, lanes=1, A=4, K=3, ref=0, loading=1e-3, target=12.0, null=None):
    taps = np.zeros(256, dtype=np.int16)
    w = np.zeros(256)
    shift, gain, supp = C.c_int32(0), C.c_double(0), C.c_double(0)
    ptrs = dict(rho=n._ptr(rho), taps=n._ptr(taps), shift=C.byref(shift), weights=n._ptr(w), gain=C.byref(gain),
                suppression_db=C.byref(supp))
    if null:
        ptrs[null] = None
    return n.lib().sgx_array_design(ptrs["rho"], frames, lanes, A, K, ref, loading, target, ptrs["taps"], ptrs["shift"],
                                    ptrs["weights"], ptrs["gain"], ptrs["suppression_db"])


def test_design_refusals(built):
    n = built._native
    rng = np.random.default_rng(7)
    rho = spec.stats(correlated_record(rng, 1000, 1, 4), 1, 4, 3)
    big = np.zeros(8 * 8 * 15 * 2, dtype=np.int64)                             # room for every shape that is refused
    big[:rho.size] = rho.ravel()
    assert _design_rc(n, big) == n.SGX_OK
    for name in ("weights", "gain", "suppression_db"):                         # optional outputs
        assert _design_rc(n, big, null=name) == n.SGX_OK

    def refused(word, contract=None, **kw):
        assert _design_rc(n, big, **kw) == n.SGX_E_ARG and word in n.last_error(), (kw, n.last_error())
        if contract is not None:
            with pytest.raises(ValueError):
                contract()

    for name in ("rho", "taps", "shift"):
        refused(name, null=name)
    for lanes in (0, 3):
        refused("lanes", lanes=lanes)
    for A in (1, 9):
        refused("A =", A=A)
    for K in (0, 2, 17):
        refused("K =", K=K)
    refused("A K", A=8, K=9)
    for ref in (-1, 4):
        refused("ref", lambda ref=ref: spec.design(rho, 1000, 1, ref), ref=ref)
    for loading in (-1e-3, np.inf, np.nan):
        refused("loading", lambda v=loading: spec.design(rho, 1000, 1, 0, v), loading=loading)
    for target in (0.0, -1.0, 127.5, np.nan):
        refused("target_rms", lambda v=target: spec.design(rho, 1000, 1, 0, 1e-3, v), target=target)
    refused("frames", lambda: spec.design(rho, 0, 1), frames=0)
    # an all-zero record: not positive definite, loading or not
    zero = np.zeros_like(big)
    for loading in (0.0, 1e-3):
        assert _design_rc(n, zero, loading=loading) == n.SGX_E_ARG and "positive definite" in n.last_error()
        with pytest.raises(ValueError, match="positive definite"):
            spec.design(np.zeros_like(rho), 1000, 1, 0, loading)
    # two streams that repeat each other, no loading: singular
    twin = np.tile(rng.integers(-50, 50, (500, 1)), (1, 2)).astype(np.int8).reshape(-1)
    with pytest.raises(ValueError, match="positive definite"):
        spec.design(spec.stats(twin, 1, 2, 1), 500, 1, 0, 0.0)
    with pytest.raises(n.SgxError, match="positive definite"):
        n.array_design(spec.stats(twin, 1, 2, 1), 500, 1, 0, 0.0)
    # a quiet record at a high target: the reference tap alone, 4096 x gain, leaves +-32512
    quiet = rng.integers(-1, 2, 4000).astype(np.int8)
    rq = spec.stats(quiet, 1, 4, 1)
    with pytest.raises(ValueError, match="tap"):
        spec.design(rq, 1000, 1, 0, 1e-3, 12.0)
    with pytest.raises(n.SgxError, match="32512"):
        n.array_design(rq, 1000, 1, 0, 1e-3, 12.0)
    # (128 sum(|re| + |im|) >= 2^31 needs sum|taps| >= 2^24; 64 complex weights at +-32512 reach 2^22: the design cannot
    # meet that refusal, which the combiner's own check of foreign taps keeps - tests/test_array_gpu.py)
    assert 2 * spec.MAX_WEIGHTS * spec.MAX_TAP * 128 < 2 ** 31
    with pytest.raises(ValueError, match="shape"):
        n.array_design(rho[:, :3], 1000, 1)


# ---- the scenes: the oracle alone ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_scenes_are_what_they_claim(name):
    """No single antenna acquires any of the four satellites; the contracts' combined record acquires all four well above
    the threshold and no other PRN comes near it - at the start of the file and behind the end-to-end skip."""
    scene = cases.SCENES[name]
    frames = cases.ACQ_MS * scene.frames_per_ms
    c = cases.combined(scene, frames)
    alone = cases.prepared_of(scene, cases.antenna(cases.head(scene, frames), scene, 0))
    present = np.array(scene.prns) - 1
    absent = np.setdiff1d(np.arange(32), present)
    threshold = scene.oracle_settings().acqThreshold
    for skip in (0, cases.SKIP_FRAMES * scene.lanes):
        a0 = cases.acquisition(scene, alone, skip)
        assert not np.any(np.asarray(a0["carrFreq"])[present]), (skip, a0["peakMetric"][present])
        assert np.all(a0["peakMetric"][present] < threshold)
        ac = cases.acquisition(scene, c["prepared"], skip)
        assert np.all(ac["peakMetric"][present] >= cases.MARGIN * threshold), (skip, ac["peakMetric"][present])
        assert np.all(ac["peakMetric"][absent] <= cases.ABSENT_MAX), (skip, ac["peakMetric"][absent].max())
        assert sorted(np.flatnonzero(ac["carrFreq"]) + 1) == sorted(scene.prns)
    # the output sits at the target: rounding adds 1/12 LSB^2 to 144; nothing clips
    rms = float(np.sqrt(np.mean(c["combined"].astype(np.float64) ** 2)))
    assert abs(rms - spec.DEFAULT_TARGET_RMS) <= 0.01 * spec.DEFAULT_TARGET_RMS, rms
    assert c["clipped"] == 0
    # the suppression the output bytes show against the design's prediction, and against the recorded figure
    measured = cases.measured_suppression_db(scene, frames)
    print("%s: suppression designed %.4f dB, measured %.4f dB" % (name, c["suppression_db"], measured))
    assert abs(measured - c["suppression_db"]) <= cases.SUPPRESSION_TOL_DB
    assert abs(measured - cases.MEASURED_SUPPRESSION_DB[name]) <= 0.01
    assert c["suppression_db"] > 14.0                                          # a null, not a gain setting
    # what the null leaves of every satellite (a direction near the jammer's loses most): the truth the end-to-end test holds
    # the prompt arms to
    print("%s: amplitudes behind the combiner %s LSB" % (name, ", ".join(
        "%.2f" % scene.amplitude_out(i, c["weights"], c["gain"]) for i in range(len(scene.prns)))))


# ---- Settings: the walk -------------------------------------------------------------------------------------------------

def test_the_stage_stands_behind_the_unpacker(built):
    f = pkg("frontend")
    names = [s.name for s in f.STAGES]
    assert names.index("combine") == names.index("unpack") + 1
    st = f.STAGES[names.index("combine")]
    assert (st.flag, st.last, st.reads, st.makes) == ("antennas", "lastCombining", "a frame of all antennas", "a frame")
    assert (st.replays_file, st.verb) == (False, "combines")
    s = built.Settings()
    assert (s.antennas, s.arrayTaps, s.arrayReference, s.arrayLoading, s.arrayTargetRms) == (0, 0, 0, 1e-3, 12.0)
    assert not st.on(s) and s._walk() == ([], s)
    n = built._native
    assert (n.ARRAY_MAX_ANTENNAS, n.ARRAY_MAX_TAPS, n.ARRAY_SHIFT) == (spec.MAX_ANTENNAS, spec.MAX_TAPS, spec.DESIGN_SHIFT)
    with pytest.raises(ValueError, match="antennas is 0"):
        s.combineAntennas(None)


def test_walk_and_file_range(built):
    real = cases.SCENE_REAL.settings(built, skipNumberOfBytes=4 * cases.SKIP_FRAMES)
    assert real._array_format() == (1, 4, 5, 0, False)
    p = real._prepared_settings()
    assert (p.antennas, p.dataType, p.skipNumberOfBytes, p.samplingFreq, p.IF) == (0, 'int8', cases.SKIP_FRAMES, real.samplingFreq, real.IF)
    assert real.antennas == 4 and real.skipNumberOfBytes == 4 * cases.SKIP_FRAMES             # left alone
    assert real._file_range(100, 1000) == (400, 4000)
    steps = real._walk()[0]
    assert [(st.name, n_in, n_out) for st, _, n_in, n_out in steps] == [("combine", 4, 1)]
    # I/Q: frames of 8 bytes become pairs; the converter stands behind
    iq = cases.SCENE_IQ.settings(built, skipNumberOfBytes=8 * cases.SKIP_FRAMES, dataType='uint8', arrayReference=3)
    assert iq._array_format() == (2, 4, 1, 3, True)
    p = iq._prepared_settings()
    assert (p.antennas, p.iqRecord, p.dataType, p.skipNumberOfBytes) == (0, False, 'int8', 2 * cases.SKIP_FRAMES)
    assert (p.samplingFreq, p.IF) == cases.SCENE_IQ.prepared_rate()
    assert [(st.name, a, b) for st, _, a, b in iq._walk()[0]] == [("combine", 8, 2), ("convert", 2, 2)]
    assert iq._file_range(2 * 50, 2 * 300) == (8 * 50, 8 * 300)
    with pytest.raises(ValueError, match="pair"):
        iq._file_range(3, 10)
    # a skip off a frame of all antennas
    for s, skip in ((real, 4 * 10 + 2), (iq, 8 * 10 + 4)):
        s.skipNumberOfBytes = skip
        with pytest.raises(ValueError, match="a frame of all antennas"):
            s._walk()


def test_chains_behind_the_stage(built):
    # the decimator: 5 frames of 4 antennas per prepared sample
    s = built.Settings()
    s.antennas, s.decimation, s.skipNumberOfBytes = 4, 5, 4 * 5 * 100
    p = s._prepared_settings()
    assert [(st.name, a, b) for st, _, a, b in s._walk()[0]] == [("combine", 4, 1), ("decimate", 5, 1)]
    assert (p.skipNumberOfBytes, p.samplingFreq) == (100, s.samplingFreq / 5) and s._file_range(10, 20) == (200, 400)
    s.skipNumberOfBytes = 4 * 7
    with pytest.raises(ValueError, match="decimat"):
        s._walk()
    # the resampler, and the notch behind everything (it changes no position)
    s = built.Settings()
    s.samplingFreq, s.IF, s.antennas, s.resampleUp, s.interferenceMitigation = 4096000.0, 1000000.0, 2, 10, True
    s.skipNumberOfBytes = 2 * 33
    p = s._prepared_settings()
    assert [(st.name, a, b) for st, _, a, b in s._walk()[0]] == [("combine", 2, 1), ("resample", 1, 10)]
    assert (p.skipNumberOfBytes, p.samplingFreq, p.interferenceMitigation) == (330, 40960000.0, True)
    # I/Q through the decimator and the converter
    s = built.Settings()
    s.samplingFreq, s.IF, s.iqRecord, s.antennas, s.decimation = 16368000.0, 3200000.0, True, 3, 4
    s.skipNumberOfBytes = 6 * 4 * 9
    assert [(st.name, a, b) for st, _, a, b in s._walk()[0]] == [("combine", 6, 2), ("decimate", 8, 2), ("convert", 2, 2)]
    assert s._prepared_settings().skipNumberOfBytes == 18


def test_array_format_refusals(built):
    def refused(word, **kw):
        s = built.Settings()
        s.antennas = 4
        for k, v in kw.items():
            setattr(s, k, v)
        with pytest.raises(ValueError, match=word):
            s._array_format()
        with pytest.raises(ValueError, match=word):
            s._walk()

    refused("frontEndConditioning", frontEndConditioning=True)
    refused("coherence", iqRecord=True, iqRequantize=True, dataType='int16')
    for dt in ('int16', 'float32', 'float64'):
        refused("dataType", dataType=dt)
    for A in (1, 9, -2, 2.5, "x"):
        refused("Settings.antennas", antennas=A)
    for K in (2, 17, -1, 4.5):
        refused("Settings.arrayTaps", arrayTaps=K)
    refused("weights", antennas=8, arrayTaps=9)
    for ref in (-1, 4, 0.5):
        refused("Settings.arrayReference", arrayReference=ref)
    for v in (-1.0, np.inf, np.nan):
        refused("Settings.arrayLoading", arrayLoading=v)
    for v in (0.0, 128.0, np.nan):
        refused("Settings.arrayTargetRms", arrayTargetRms=v)
    s = built.Settings()
    s.antennas, s.iqRecord = 8, True
    assert s._array_format()[:3] == (2, 8, 1)
    s.iqRecord, s.arrayTaps = False, 7
    assert s._array_format()[:3] == (1, 8, 7)


def test_the_unpacker_takes_the_streams_of_all_antennas(built):
    s = built.Settings()
    s.packedBits, s.packedFrame = 4, 4
    assert s._pack_format()[4] == 1 and s._pack_units() == (2, 1)              # without antennas nothing changes
    s.antennas = 4
    assert s._pack_format()[2:5] == (4, 0, 4) and s._pack_units() == (2, 4)
    assert [(st.name, a, b) for st, _, a, b in s._walk()[0]] == [("unpack", 2, 4), ("combine", 4, 1)]
    s.skipNumberOfBytes = 2 * 11
    assert s._prepared_settings().skipNumberOfBytes == 11 and s._file_range(11, 100) == (22, 200)
    s.skipNumberOfBytes = 0
    s.antennas, s.packedFirst = 2, 2                                           # two of the four streams, from field 2 on
    assert s._pack_format()[2:5] == (4, 2, 2)
    s.packedFirst = 3
    with pytest.raises(ValueError, match="packedFirst"):
        s._pack_format()
    s.packedFirst, s.iqRecord, s.packedFrame, s.packedBits = 0, True, 8, 2    # I/Q pairs of two antennas out of eight fields
    assert s._pack_format()[2:5] == (8, 0, 4) and s._pack_units() == (2, 4)
    s.antennas = 8
    with pytest.raises(ValueError, match="packedFirst"):
        s._pack_format()
    s.antennas, s.packedFrame = 4, 1                                           # one field per frame: every field is taken
    assert s._pack_format()[4] == 1


# ---- the command line ---------------------------------------------------------------------------------------------------

def test_options(built, monkeypatch, capsys):
    main = pkg("main")
    seen = {}

    def fake_post(self, fileNameStr=None):
        seen.clear()
        seen.update(A=self.antennas, K=self.arrayTaps, ref=self.arrayReference, loading=self.arrayLoading,
                    target=self.arrayTargetRms, iq=self.iqRecord, dataType=self.dataType, skip=self.skipNumberOfBytes)
        return None, None, None

    monkeypatch.setattr(built.Settings, "postProcessing", fake_post)
    assert main.main(["x.bin", "--no-probe", "--fs", "16368000", "--IF", "4092000", "--antennas", "4:1", "--array-taps", "5",
                      "--skip", "400"]) == 0
    assert seen == dict(A=4, K=5, ref=1, loading=1e-3, target=12.0, iq=False, dataType="int8", skip=400)
    out = capsys.readouterr().out
    assert "Combined 4 antennas: read as a real record at 16.368000 Msps, IF 4.092000 MHz" in out
    assert main.main(["x.bin", "--no-probe", "--iq", "--fs", "4092000", "--IF", "0", "--dtype", "uint8", "--antennas", "8"]) == 0
    assert seen == dict(A=8, K=0, ref=0, loading=1e-3, target=12.0, iq=True, dataType="uint8", skip=0)
    assert "read as a real record at 8.184000 Msps, IF 2.046000 MHz" in capsys.readouterr().out
    assert main.main(["x.bin", "--no-probe", "--packed", "4", "--packed-frame", "4", "--antennas", "4"]) == 0
    assert seen["A"] == 4
    assert main.main(["x.bin", "--no-probe"]) == 0
    assert seen["A"] == 0
    for option in ("--antennas", "--array-taps"):
        assert option in main.__doc__


REFUSED = [
    ["x.bin", "--array-taps", "5"], ["x.bin", "--antennas", "1"], ["x.bin", "--antennas", "9"], ["x.bin", "--antennas", "0"],
    ["x.bin", "--antennas", "x"], ["x.bin", "--antennas", "4:4"], ["x.bin", "--antennas", "4:1:2"],
    ["x.bin", "--antennas", "4", "--array-taps", "4"], ["x.bin", "--antennas", "4", "--array-taps", "0"],
    ["x.bin", "--antennas", "4", "--array-taps", "17"], ["x.bin", "--antennas", "8", "--array-taps", "9"],
    ["x.bin", "--antennas", "4", "--condition"], ["x.bin", "--antennas", "4", "--iq", "--dtype", "int16", "--iq-requantize"],
    ["x.bin", "--antennas", "4", "--dtype", "int16"], ["x.bin", "--antennas", "4", "--correlator-bank", "0:1:0.5"],
    ["x.bin", "--packed", "4", "--packed-frame", "4:1", "--antennas", "4"],
]


@pytest.mark.parametrize("argv", REFUSED, ids=[" ".join(a[1:]) for a in REFUSED])
def test_refused_as_a_usage_error(built, monkeypatch, capsys, argv):
    def never(self, *args, **kw):
        raise AssertionError("the run went on")

    for method in ("postProcessing", "probeData", "_prepared_record"):
        monkeypatch.setattr(built.Settings, method, never)
    with pytest.raises(SystemExit) as e:
        pkg("main").main(argv)
    assert e.value.code == 2
    captured = capsys.readouterr()
    message = captured.err.split(": error: ", 1)[1]
    f = pkg("frontend")
    stages = dict((s.name, s) for s in f.STAGES)
    words = [flag for name in ("combine", "unpack") for flag, _ in stages[name].options] + \
        ["Settings." + k for name in ("combine", "unpack") for k, _ in stages[name].defaults]
    assert any(w in message for w in words), message
    assert "Welcome" not in captured.out and "Traceback" not in captured.err


def test_a_skip_off_a_frame_is_a_usage_error(built, monkeypatch, capsys):
    monkeypatch.setattr(built.Settings, "postProcessing", lambda self, fileNameStr=None: (None, None, None))
    with pytest.raises(SystemExit) as e:
        pkg("main").main(["x.bin", "--no-probe", "--antennas", "4", "--skip", "6"])
    assert e.value.code == 2 and "a frame of all antennas" in capsys.readouterr().err
