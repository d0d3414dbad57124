"""CPU-only checks of the resampling stage (include/sgx.h: sgx_resamp_design, and the argument refusals of sgx_if_resample
that need no record) against the numpy contract of tests/resamp_spec.py; the contract's own closed forms and the agreement
of its two forms; the image rejection of the default design; which tracking kernel and which FFT length a resampled record
reaches; the Settings surface and the skip arithmetic; and the scenes of tests/resamp_cases.py shown to
be well conditioned by the contract plus the oracle alone."""
import ctypes as C
import importlib

import numpy as np
import pytest

import resamp_cases as cases
import resamp_spec as spec
from conftest import pkg

MARGIN = 1e-9
# Rejection by the default design (24 L + 1 taps, default cutoff) of the strongest image of a full-scale tone, against the
# tone itself, measured on the contract (test_image_rejection_of_the_default_design prints them).  The tone sits in the
# band where its first image, fs - f, falls on the edge of the design's stopband, fc + 2 fu / (Lh - 1), and up to one
# sidelobe width beyond it - five placements, the worst one counts: the design bound of 44 dB, met.  Tones above that edge
# (the outer 0.3 MHz of a C/A band at 4.096 Msps with the IF at 1.0 MHz) have their first image in the transition band.
IMAGE_REJECTION_DB = {(4096000.0, 10, 1): 44.2, (16368000.0, 7, 3): 44.8, (2048000.0, 8, 1): 45.7, (8192000.0, 5, 1): 44.6}

# (fs, L, M, Lh, cutoff, gain): the rates of the issue's list, every M, L = 2 and 16, Lh = 1, the default and 1023, cutoffs
# below the default, gains either side of 1
GRID = [
    (4096000.0, 10, 1, 241, 0.0, 1.0),
    (16368000.0, 7, 3, 169, 0.0, 1.0),
    (2048000.0, 8, 1, 193, 0.0, 1.0),
    (8192000.0, 5, 1, 121, 0.0, 1.0),
    (5456000.0, 7, 1, 169, 0.0, 1.0),
    (2400000.0, 16, 1, 385, 1100000.0, 1.0),
    (2048000.0, 8, 1, 65, 900000.0, 1.3),
    (8192000.0, 5, 1, 1023, 0.0, 1.0),
    (5456000.0, 7, 1, 1, 0.0, 1.0),
    (4000000.0, 16, 3, 301, 1100000.0, 0.7),
    (8184000.0, 14, 3, 337, 0.0, 1.0),
    (16368000.0, 5, 2, 121, 7000000.0, 1.9),
    (4092000.0, 3, 2, 73, 0.0, 0.5),
    (4096000.0, 2, 1, 49, 2000000.0, 1.0),
]


@pytest.fixture(scope="module")
def built():
    importlib.import_module("__graft_entry__").build()
    return pkg()


# ---- the design function ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", GRID, ids=["%g-%d_%d-L%d" % (g[0] / 1e6, g[1], g[2], g[3]) for g in GRID])
def test_design_equals_the_contract(built, args):
    fs, L, M, Lh, cutoff, gain = args
    margin = spec.rounding_margin(*args)
    assert margin > MARGIN, "an unrounded tap of this case sits on a rounding boundary (%.3g): pick another" % margin
    taps, shift, info = built._native.resamp_design(fs, L, M, Lh, cutoff, gain)
    want, want_shift, fs_out = spec.design(*args)
    assert shift == want_shift == spec.DESIGN_SHIFT == built._native.RESAMP_SHIFT
    assert taps.dtype == np.int16 and taps.size == Lh and np.array_equal(taps, want)
    assert info["fs_out"] == fs_out == fs * L / M                              # exactly
    spec.check(taps, shift, L, M)                                              # what it designs, the resampler takes


def test_default_length_and_the_rates_of_the_issue(built):
    n = built._native
    for fs, L, M, fo in ((5456000.0, 7, 1, 38192000.0), (16368000.0, 7, 3, 38192000.0), (4096000.0, 10, 1, 40960000.0),
                         (2048000.0, 8, 1, 16384000.0), (8192000.0, 5, 1, 40960000.0)):
        taps, shift, info = n.resamp_design(fs, L, M)
        assert taps.size == 24 * L + 1 == spec.default_taps(L) and info["fs_out"] == fo and shift == 14
        assert np.array_equal(taps, spec.design(fs, L, M)[0])
        if M == 1:                                                             # phase 0 is the single tap 2^14
            phase0 = taps[(taps.size - 1) // 2 % L::L]
            assert np.count_nonzero(phase0) == 1 and phase0.max() == 1 << 14 and taps[(taps.size - 1) // 2] == 1 << 14
    assert n.RESAMP_MAX_TAPS == spec.MAX_TAPS == 1023 and (n.RESAMP_MAX_UP, n.RESAMP_MAX_DOWN) == (16, 3)
    assert sum(n.resamp_pair_ok(L, M) for L in range(0, 20) for M in range(0, 6)) == 31
    assert all(n.resamp_pair_ok(L, M) for L, M in spec.PAIRS)


def _design_rc(n, fs=4096000.0, L=10, M=1, Lh=241, cutoff=0.0, gain=1.0, null=None):
    taps = np.zeros(1100, dtype=np.int16)
    shift, fo = C.c_int32(0), C.c_double(0)
    ptrs = dict(taps=n._ptr(taps), shift=C.byref(shift), fs_out=C.byref(fo))
    if null:
        ptrs[null] = None
    return n.lib().sgx_resamp_design(fs, L, M, Lh, cutoff, gain, ptrs["taps"], ptrs["shift"], ptrs["fs_out"])


def test_design_refusals(built):
    n = built._native
    assert _design_rc(n) == n.SGX_OK

    def refused(word, contract=True, **kw):
        assert _design_rc(n, **kw) == n.SGX_E_ARG and word in n.last_error(), (kw, n.last_error())
        if contract:
            a = dict(fs=4096000.0, L=10, M=1, Lh=241, cutoff=0.0, gain=1.0)
            a.update(kw)
            with pytest.raises(ValueError):
                spec.design(a["fs"], a["L"], a["M"], a["Lh"] if a["Lh"] else -1, a["cutoff"], a["gain"])

    for name in ("taps", "shift", "fs_out"):
        refused(name, contract=False, null=name)
    for fs in (0.0, -1.0, np.inf, np.nan):
        refused("fs", fs=fs)
    for gain in (0.0, -1.0, np.inf, np.nan):
        refused("gain", gain=gain)
    for L, M in ((1, 1), (17, 1), (0, 1), (4, 2), (6, 3), (3, 3), (2, 3), (5, 4), (5, 0), (-3, 1)):
        refused("L / M", L=L, M=M)
    for Lh in (0, 2, 240, 1025, -1):
        refused("n_taps", Lh=Lh)
    for cutoff in (-1.0, np.inf, np.nan, 2048001.0, 3e6):                      # above min(fs, fs_out) / 2
        refused("cutoff_hz", cutoff=cutoff)
    refused("cutoff_hz", fs=16368000.0, L=7, M=3, Lh=169, cutoff=8184001.0)
    assert _design_rc(n, cutoff=2048000.0) == n.SGX_OK
    # a tap beyond what the resampler takes: the centre tap is 2^14 g (M = 1, default cutoff)
    refused("32512", gain=2.0)
    assert _design_rc(n, gain=1.98) == n.SGX_OK
    assert n.lib().sgx_resamp_timing(None, None) == n.SGX_E_ARG
    assert n.lib().sgx_resamp_tile(None) == n.SGX_E_ARG
    assert n.resamp_tile() > 0 and n.resamp_tile() % 256 == 0


# ---- the resampler's refusals that need no record -----------------------------------------------------------------------

def _resample_rc(n, taps, n_taps=None, shift=14, L=4, M=1, null_taps=False):
    h = np.ascontiguousarray(taps, dtype=np.int16)
    out = C.c_void_p()
    return n.lib().sgx_if_resample(None, None, None if null_taps else n._ptr(h), h.size if n_taps is None else n_taps, shift,
                                   L, M, C.byref(out), None)


def test_resampler_refuses_bad_arguments_before_it_looks_at_the_device(built):
    """Every precondition of the contract that needs no record: each refusal is SGX_E_ARG and names its own argument (and
    the contract's check() raises on it); good arguments get as far as the missing context."""
    n = built._native
    good = np.arange(-31, 32, dtype=np.int16)
    far = "c && rec && out"
    for L, M in spec.PAIRS:
        assert _resample_rc(n, good, L=L, M=M) == n.SGX_E_ARG and far in n.last_error()
        spec.check(good, 14, L, M)
    bad_pairs = [(L, M) for L in range(-1, 19) for M in range(-1, 6) if (L, M) not in spec.PAIRS]
    assert len(bad_pairs) == 20 * 7 - 31
    for L, M in bad_pairs:
        assert _resample_rc(n, good, L=L, M=M) == n.SGX_E_ARG and "L / M = %d / %d" % (L, M) in n.last_error()
        with pytest.raises(ValueError):
            spec.check(good, 14, L, M)
    for Lh in (0, 2, 62, 1024, 1025, -1):
        assert _resample_rc(n, np.zeros(1100, dtype=np.int16), n_taps=Lh) == n.SGX_E_ARG and "n_taps" in n.last_error(), Lh
        if Lh > 0:
            with pytest.raises(ValueError):
                spec.check(np.zeros(Lh, dtype=np.int16), 14, 4, 1)
    assert _resample_rc(n, np.zeros(1023, dtype=np.int16)) == n.SGX_E_ARG and far in n.last_error()
    for shift in (-1, 31):
        assert _resample_rc(n, good, shift=shift) == n.SGX_E_ARG and "shift" in n.last_error()
        with pytest.raises(ValueError):
            spec.check(good, shift, 4, 1)
    for shift in (0, 30):
        assert _resample_rc(n, good, shift=shift) == n.SGX_E_ARG and far in n.last_error()
    assert _resample_rc(n, good, null_taps=True) == n.SGX_E_ARG and "taps" in n.last_error()
    for v in (32513, -32513, 32767, -32768):
        big = good.copy()
        big[3] = v
        assert _resample_rc(n, big) == n.SGX_E_ARG and "32512" in n.last_error(), v
        with pytest.raises(ValueError):
            spec.check(big, 14, 4, 1)
    for v in (32512, -32512):
        big = good.copy()
        big[3] = v
        assert _resample_rc(n, big) == n.SGX_E_ARG and far in n.last_error(), v
    # 128 sum|h| < 2^31: within reach of 1023 taps
    budget = (2 ** 31 - 1) // 128
    h = np.zeros(1023, dtype=np.int16)
    h[:budget // 32512] = 32512
    h[budget // 32512] = budget - 32512 * (budget // 32512)
    assert 128 * int(np.abs(h.astype(np.int64)).sum()) == 2 ** 31 - 128
    assert _resample_rc(n, h) == n.SGX_E_ARG and far in n.last_error()
    spec.check(h, 0, 4, 1)
    h[-1] = -1                                                                 # one more LSB
    assert _resample_rc(n, h) == n.SGX_E_ARG and "2^31" in n.last_error()
    with pytest.raises(ValueError):
        spec.check(h, 0, 4, 1)


# ---- the contract's own properties --------------------------------------------------------------------------------------

def test_the_two_forms_of_the_contract_agree():
    """resamp_spec sums stream by stream; the sums as the contract writes them, tap by tap over the stuffed record, are the
    same - on records shorter than the filter too."""
    rng = np.random.default_rng(31)
    for L, M in ((2, 1), (3, 2), (7, 3), (10, 1), (16, 3), (16, 1), (5, 2)):
        for Lh in sorted(set([1, 3, (L - 1) | 1, 2 * L + 1, 24 * L + 1, 1023])):
            for N in (0, 1, M - 1, M, M + 1, 7, 200, 201):
                x = rng.integers(-128, 128, max(N, 0)).astype(np.int64)
                h = rng.integers(-3000, 3000, Lh).astype(np.int64)
                a, b = spec.sums_direct(x, h, L, M), spec.sums_phased(x, h, L, M)
                assert a.size == b.size == spec.out_length(x.size, L, M) and np.array_equal(a, b), (L, M, Lh, N)
    b8 = rng.integers(-128, 128, 500).astype(np.int8)
    h16 = rng.integers(-300, 301, 49).astype(np.int16)
    y0, c0 = spec.resample(b8, h16, 9, 7, 3)
    y1, c1 = spec.resample(b8, h16, 9, 7, 3, direct=True)
    assert np.array_equal(y0, y1) and c0 == c1


def test_contract_closed_forms():
    rng = np.random.default_rng(32)
    b = rng.integers(-128, 128, 4001).astype(np.int8)
    x = np.clip(b.astype(np.int64), -127, 127)
    for L in (2, 5, 16):
        for S in (0, 7, 14):
            # Lh = 1, h = [2^shift]: the record with L - 1 zeros behind every sample, -128 clipped
            y, clipped = spec.resample(b, np.array([1 << S], dtype=np.int16), S, L, 1)
            assert y.size == b.size * L and np.array_equal(y[::L], x) and clipped == np.count_nonzero(b == -128)
            assert not np.any(y.reshape(-1, L)[:, 1:])
        # the default design at M = 1: phase 0 is the single tap 2^14, so every L-th output is the input
        h, S, _ = spec.design(4096000.0, L, 1)
        y, _ = spec.resample(b, h, S, L, 1)
        assert np.array_equal(y[::L], x)
    # M > 1: output m of the one-tap filter is u[m M]: x[m M / L] where L divides m M
    y, _ = spec.resample(b, np.array([1], dtype=np.int16), 0, 7, 3)
    assert y.size == -(-b.size * 7 // 3)
    m = np.arange(y.size)
    hit = (m * 3) % 7 == 0
    assert np.array_equal(y[hit], x[(m[hit] * 3) // 7]) and not np.any(y[~hit])
    # a DC input comes out within +-1 LSB of itself away from the ends, at every pair
    for L, M in spec.PAIRS:
        h, S, _ = spec.design(4096000.0, L, M)
        for level in (100, -77, 1):
            y, clipped = spec.resample(np.full(600, level, dtype=np.int8), h, S, L, M)
            mid = y[h.size:-h.size].astype(np.int64)
            assert mid.size > 100 and np.abs(mid - level).max() <= 1 and clipped == 0, (L, M, level)
    # rounding: half up before the floor shift
    y, _ = spec.resample(np.array([1, 3, -1, -3], dtype=np.int8), np.array([1], dtype=np.int16), 1, 2, 1)
    assert list(y[::2]) == [1, 2, 0, -1]
    # zero phase: an input offset that is a multiple of M is the output offset offset L / M
    h, S, _ = spec.design(16368000.0, 7, 3)
    whole, _ = spec.resample(b, h, S, 7, 3)
    tail, _ = spec.resample(b[300:], h, S, 7, 3)
    assert np.array_equal(tail[h.size:], whole[700 + h.size:])


def _spectrum(y):
    """(frequencies in cycles per sample, power) of a record under a Blackman-Harris window."""
    z = y.astype(np.float64)
    n = z.size
    k = np.arange(n)
    w = (0.35875 - 0.48829 * np.cos(2 * np.pi * k / n) + 0.14128 * np.cos(4 * np.pi * k / n)
         - 0.01168 * np.cos(6 * np.pi * k / n))
    return np.fft.rfftfreq(n), np.abs(np.fft.rfft(z * w)) ** 2


def image_rejection_db(fs, L, M, f0, n_in=12288):
    """The strongest image of a full-scale tone at f0 in the output spectrum of the default design, in dB below the tone:
    the stuffed record holds the tone at k fs +- f0, the filter is to leave k = 0 alone, and decimation by M folds what is
    left of the others into the output band."""
    h, S, fo = spec.design(fs, L, M)
    x = np.rint(127.0 * np.cos(2 * np.pi * f0 / fs * np.arange(n_in) + 0.4)).astype(np.int8)
    y = spec.resample(x, h, S, L, M)[0][h.size:-h.size]
    _, p = _spectrum(y)
    n = y.size

    def near(fr, w=6):
        k = int(round(fr * n))
        return p[max(0, k - w):min(p.size, k + w + 1)].max()

    def fold(f_hz):
        r = (f_hz / fo) % 1.0
        return min(r, 1.0 - r)

    tone_at = fold(f0)
    worst = 0.0
    for k in range(0, L + 1):
        for f in (k * fs + f0, k * fs - f0):
            if 0 < f <= fs * L / 2 and not (k == 0) and abs(fold(f) - tone_at) * n >= 16:
                worst = max(worst, near(fold(f)))
    return 10.0 * np.log10(near(tone_at) / worst)


@pytest.mark.parametrize("key", sorted(IMAGE_REJECTION_DB), ids=lambda k: "%g-%d_%d" % (k[0] / 1e6, k[1], k[2]))
def test_image_rejection_of_the_default_design(key):
    fs, L, M = key
    h, _, fo = spec.design(fs, L, M)
    fu = fs * L
    edge = min(fs, fo) / 2.0 + 2.0 * fu / (h.size - 1)                         # where the design's stopband starts
    worst = np.inf
    for j in range(5):
        f0 = fs - (edge + j * 0.25 * fu / (h.size - 1))                        # the first image, fs - f0, from the edge on
        assert 0 < f0 < fs / 2
        db = image_rejection_db(fs, L, M, f0)
        print("image rejection, %g Msps x %d/%d, tone at %.4f MHz: %.2f dB" % (fs / 1e6, L, M, f0 / 1e6, db))
        worst = min(worst, db)
    assert worst >= IMAGE_REJECTION_DB[key] - 0.5, worst
    assert worst >= 40.0, worst


# ---- what a resampled record reaches ------------------------------------------------------------------------------------

def test_kernel_selection_and_fft_length(built):
    """Through the existing selection rule (sgx_track_plan; kernel 2 trk2_kernel, 4 trk_kernel_multi, 5 trk3_kernel): the
    captures of the issue leave the per-sample kernel, and the resampled 4.096 Msps code length factors - no padded search."""
    n = built._native
    s = built.Settings()
    s.samplingFreq, s.IF = 4096000.0, 1000000.0
    assert n.track_plan(s, n.DT_INT8, 8, 256)[0] == 4
    s.resampleUp = 10
    real = s._prepared_settings()
    assert real.samplingFreq == 40960000.0 and real.samplesPerCode == 40960
    assert n.track_plan(real, n.DT_INT8, 8, 256)[0] == 5
    assert n.acquire_fft_length(real.samplesPerCode) == real.samplesPerCode == 40960
    s.samplingFreq, s.IF, s.resampleUp, s.resampleDown = 16368000.0, 4092000.0, 7, 3
    real = s._prepared_settings()
    assert real.samplingFreq == 38192000.0 and n.track_plan(real, n.DT_INT8, 8, 256)[0] == 5
    s.samplingFreq, s.IF, s.resampleUp, s.resampleDown = 2048000.0, 0.0, 8, 1
    real = s._prepared_settings()
    assert real.samplingFreq == 16384000.0 and n.track_plan(real, n.DT_INT8, 8, 256)[0] == 2


# ---- the Settings surface -----------------------------------------------------------------------------------------------

def _settings(built, fs=4096000.0, IF=1000000.0, L=10, M=1):
    s = built.Settings()
    s.samplingFreq, s.IF, s.resampleUp, s.resampleDown = fs, IF, L, M
    return s


def test_settings_surface(built):
    s = built.Settings()
    assert (s.resampleUp, s.resampleDown, s.resampTaps, s.resampCutoff, s.resampGain) == (0, 1, 0, 0.0, 1.0)
    assert s._prepared_settings() is s                                         # off: a plain record is read as it is
    with pytest.raises(ValueError, match="resampleUp"):
        s.resampleRecord(None)
    s = _settings(built)
    real = s._prepared_settings()
    assert real is not s and (real.samplingFreq, real.IF, real.resampleUp, real.dataType) == (40960000.0, 1000000.0, 0, 'int8')
    assert (s.samplingFreq, s.IF, s.resampleUp) == (4096000.0, 1000000.0, 10)  # left alone
    assert s._resamp_format() == (10, 1, 241)
    taps, shift, info = s._resamp_design()
    want = spec.design(4096000.0, 10, 1)
    assert np.array_equal(taps, want[0]) and shift == want[1] and info["fs_out"] == want[2] and info["cutoff"] == 2048000.0
    s.resampTaps, s.resampCutoff, s.resampGain = 121, 2040000.0, 1.5
    taps, shift, info = s._resamp_design()
    assert np.array_equal(taps, spec.design(4096000.0, 10, 1, 121, 2040000.0, 1.5)[0]) and s._resamp_format() == (10, 1, 121)
    # every refused combination names its setting
    s = _settings(built)
    for L, M in ((1, 1), (17, 1), (4, 2), (6, 3), (2, 3), (10, 4), (10, 0), (2.5, 1), ("x", 1), (10, 1.5)):
        s.resampleUp, s.resampleDown = L, M
        with pytest.raises(ValueError, match="resampleUp"):
            s.postProcessing("/nonexistent/record.bin")
    s = _settings(built)
    for Lh in (2, 1025, -1, 63.5, "x"):
        s.resampTaps = Lh
        with pytest.raises(ValueError, match="resampTaps"):
            s.postProcessing("/nonexistent/record.bin")
    s = _settings(built)
    for cutoff in (-1.0, 3e6, float("nan")):                                   # not a cutoff of this pair at this rate
        s.resampCutoff = cutoff
        with pytest.raises(ValueError, match="resampCutoff"):
            s.postProcessing("/nonexistent/record.bin")
    s.resampCutoff = 2023000.0                                                 # the band edge IF + 1.023 MHz at the cutoff
    with pytest.raises(ValueError, match="resampCutoff"):
        s.postProcessing("/nonexistent/record.bin")
    s.resampCutoff = 0.0
    s.IF = 1025000.0                                                           # ... and above the default cutoff
    with pytest.raises(ValueError, match="resampCutoff"):
        s._prepared_settings()
    s = _settings(built)
    for gain in (0.0, -1.0, 2.0):
        s.resampGain = gain
        with pytest.raises(ValueError, match="resampGain"):
            s.postProcessing("/nonexistent/record.bin")
    s = _settings(built)
    for dt in ('uint8', 'int16', 'float32', 'float64'):                        # a real record is int8 where the stage sees it
        s.dataType = dt
        with pytest.raises(ValueError, match="dataType"):
            s.postProcessing("/nonexistent/record.bin")
    # ... which the conditioning stage and the unpacker see to
    s.frontEndConditioning = True
    for dt in ('uint8', 'int16', 'int8'):
        s.dataType = dt
        real = s._prepared_settings()
        assert (real.dataType, real.frontEndConditioning, real.resampleUp, real.samplingFreq) == ('int8', False, 0, 40960000.0)
    s.frontEndConditioning, s.dataType, s.packedBits = False, 'int8', 2
    real = s._prepared_settings()
    assert (real.packedBits, real.resampleUp, real.samplingFreq) == (0, 0, 40960000.0)
    # an I/Q capture is resampled as the real record the converter makes of it: an RTL-SDR at 2.048 Msps complex is a real
    # record at 4.096 Msps with the IF at 1.024 MHz, and comes out at 40.96 Msps
    s = _settings(built, fs=2048000.0, IF=0.0)
    s.iqRecord, s.dataType = True, 'uint8'
    real = s._prepared_settings()
    assert (real.samplingFreq, real.IF, real.iqRecord, real.dataType, real.resampleUp) == (40960000.0, 1024000.0, False, 'int8', 0)
    assert s._resamp_design()[2]["cutoff"] == 2048000.0
    # behind the decimator: the default record by 5, then 5 / 1 back up
    s = built.Settings()
    s.decimation, s.resampleUp = 5, 5
    real = s._prepared_settings()
    assert (real.samplingFreq, real.decimation, real.resampleUp) == (38192000.0, 0, 0) and abs(real.IF - 1909600.0) < 1e-6


def test_skip_arithmetic(built):
    """skipNumberOfBytes is a byte of the file; behind the stages in front it is a sample of the record the resampler reads,
    on a multiple of M, and becomes that sample L / M of the prepared record."""
    for fs, IF, L, M in ((4096000.0, 1000000.0, 10, 1), (16368000.0, 4092000.0, 7, 3), (8184000.0, 2000000.0, 14, 3),
                         (16368000.0, 4092000.0, 5, 2)):
        s = _settings(built, fs, IF, L, M)
        for k in (0, 1, 5, 1237):
            s.skipNumberOfBytes = k * M
            real = s._prepared_settings()
            assert real.skipNumberOfBytes == k * L and real.samplingFreq == fs * L / M and real.IF == IF
            assert s.skipNumberOfBytes == k * M
        for skip in (1, M - 1, M + 1, 7 * M + 1):
            if skip % M:
                s.skipNumberOfBytes = skip
                with pytest.raises(ValueError, match="skipNumberOfBytes = %d" % skip):
                    s._prepared_settings()
                with pytest.raises(ValueError, match="skipNumberOfBytes = %d" % skip):
                    s.postProcessing("/nonexistent/record.bin")
    # behind the conditioning stage of an int16 file: byte 2 k M of the file
    s = _settings(built, 16368000.0, 4092000.0, 7, 3)
    s.frontEndConditioning, s.dataType, s.skipNumberOfBytes = True, 'int16', 2 * 3 * 11
    assert s._prepared_settings().skipNumberOfBytes == 7 * 11
    s.skipNumberOfBytes = 2 * 4
    with pytest.raises(ValueError, match="skipNumberOfBytes = 8"):
        s._prepared_settings()
    # behind the I/Q converter: a byte of the file is a sample of the real record
    s = _settings(built, 2048000.0, 0.0, 10, 1)
    s.iqRecord, s.skipNumberOfBytes = True, 2 * 321
    assert s._prepared_settings().skipNumberOfBytes == 10 * 2 * 321
    # a prepared-record offset is a multiple of L: the record behind it starts on a whole sample
    s = _settings(built)
    with pytest.raises(ValueError, match="resampleUp"):
        with s._prepared_record("/nonexistent/record.bin", 7, 100):
            pass
    for case in cases.CASES.values():
        s = case.settings(built, skipNumberOfBytes=case.skip_in(cases.SKIP_UNITS))
        real = s._prepared_settings()
        assert real.skipNumberOfBytes == case.skip_out(cases.SKIP_UNITS)
        assert (real.samplingFreq, real.IF) == (case.fs_out, case.scene.f0)


# ---- the scenes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_scenes_are_well_conditioned(name):
    """The contract's record under the oracle's search: exactly the scene's satellites, where the scene put them, each at
    least MARGIN above the threshold, and every one of the 28 absent PRNs at or below ABSENT_MAX: the precondition of the
    end-to-end tests on the GPU, which leave nothing out."""
    case = cases.CASES[name]
    scene = case.scene
    o = case.oracle_settings()
    y, clipped = cases.prepared(case, cases.ACQ_MS)
    assert y.size == spec.out_length(cases.ACQ_MS * scene.frames_per_ms, case.L, case.M)
    a = np.abs(y.astype(np.int64))
    win = np.concatenate(([0], np.cumsum(a)))
    print("%s: rms %.2f, max |y| %d, %d clipped, largest 2048-sample sum of magnitudes %d"
          % (name, float(np.sqrt(np.mean(y.astype(np.float64) ** 2))), a.max(), clipped, (win[2048:] - win[:-2048]).max()))
    assert (win[2048:] - win[:-2048]).max() < 131072                           # tracking stays on its fastest kernel
    n = o.samplesPerCode
    for units in (0, cases.SKIP_UNITS):                                        # the two windows the GPU tests acquire in
        ref = cases.contract_acquisition(case, units)
        assert sorted(np.flatnonzero(ref["carrFreq"]) + 1) == sorted(scene.prns)
        absent = [p for p in range(1, 33) if p not in scene.prns]
        assert len(absent) == 28
        others = np.asarray(ref["peakMetric"])[[p - 1 for p in absent]]
        print("%s, skip %d: largest peak metric among the 28 absent PRNs %.3f" % (name, units, float(others.max())))
        assert others.max() <= cases.ABSENT_MAX
        for i, prn in enumerate(scene.prns):
            f, c, pm = ref["carrFreq"][prn - 1], ref["codePhase"][prn - 1], ref["peakMetric"][prn - 1]
            off = (c - (case.true_phase(i) - case.skip_out(units)) + n / 2.0) % n - n / 2.0
            print("%s, skip %d, PRN %2d: carrFreq %+.1f Hz, code phase %+.2f samples off the truth, peak metric %.1f"
                  % (name, units, prn, f - case.true_carrier(i), off, pm))
            assert abs(f - case.true_carrier(i)) <= cases.CARR_TOL_HZ
            assert abs(off) <= cases.PHASE_TOL * case.L / case.M
            assert pm >= cases.MARGIN * o.acqThreshold
