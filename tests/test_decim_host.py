"""CPU-only checks of the decimation stage (include/sgx.h: sgx_decim_design, and the argument refusals of sgx_if_decimate
that need no record) against the numpy contract of tests/decim_spec.py; the contract's own properties - where a tone comes
out, what an aliasing zone leaves, the Q-first identity; the Settings surface and the skip arithmetic;
and the scenes of tests/decim_cases.py shown to be well conditioned by the contracts plus the oracle alone."""
import ctypes as C
import importlib

import numpy as np
import pytest

import decim_cases as cases
import decim_spec as spec
from conftest import pkg

MARGIN = 1e-9
# Rejection by the default 127-tap design of the weakest tone that aliases into the kept band (f_out +- 0.4 bandwidth),
# against the wanted tone at the same output frequency, measured on the contract
# (test_alias_rejection_of_the_default_design prints them): D = 3 and 5 on the default record (real, 38.192 Msps, IF
# 9.548 MHz); where that record's IF sits on a zone edge, D = 4 on scene a's I/Q capture (16.368 Msps, carrier at +3.2 MHz)
# and D = 8 on a real record at 40 Msps, IF 6.2 MHz.  3 dB are taken off for the placement of a tone between two bins.
ALIAS_REJECTION_DB = {3: 48.9, 4: 52.2, 5: 46.6, 8: 40.6}

# (fs, f0, bandwidth, lanes, D, L, gain): zones 0 .. 5 of a real record, the I/Q wrap on both sides, L = 1 and L = 511
GRID = [
    (38192000.0, 9548000.0, 2046000.0, 1, 5, 127, 0.0),
    (38192000.0, 9548000.0, 2046000.0, 1, 3, 127, 0.0),
    (38192000.0, 9548000.0, 2046000.0, 1, 5, 511, 0.0),
    (38192000.0, 9548000.0, 2046000.0, 1, 3, 1, 0.0),
    (40000000.0, 1300000.0, 2046000.0, 1, 8, 63, 0.0),            # zone 0
    (40000000.0, 3800000.0, 2046000.0, 1, 8, 63, 2.5),            # zone 1
    (40000000.0, 6200000.0, 2046000.0, 1, 8, 255, 0.0),           # zone 2
    (40000000.0, 8900000.0, 2000000.0, 1, 8, 31, 1.0),            # zone 3
    (40000000.0, 11200000.0, 2046000.0, 1, 8, 127, 0.0),          # zone 4
    (40000000.0, 13700000.0, 2046000.0, 1, 8, 511, 0.0),          # zone 5
    (53000000.0, 20100000.0, 4000000.0, 1, 2, 95, 0.0),
    (16368000.0, 3200000.0, 2046000.0, 2, 4, 63, 0.0),            # wraps below -fs_out / 2: -0.892 MHz
    (16368000.0, 3200000.0, 2046000.0, 2, 4, 127, 0.0),
    (16368000.0, -3200000.0, 2046000.0, 2, 4, 127, 0.0),          # wraps the other way: +0.892 MHz
    (16368000.0, -200000.0, 2046000.0, 2, 2, 1, 0.0),
    (25000000.0, 7100000.0, 2046000.0, 2, 10, 511, 0.0),
    (25000000.0, -11900000.0, 2400000.0, 2, 10, 201, 3.0),
    (10000000.0, 0.0, 2046000.0, 2, 3, 77, 0.0),
]


@pytest.fixture(scope="module")
def built():
    importlib.import_module("__graft_entry__").build()
    return pkg()


# ---- the design function ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", GRID, ids=["%g-%g-%d-D%d-L%d" % (g[0] / 1e6, g[1] / 1e6, g[3], g[4], g[5]) for g in GRID])
def test_design_equals_the_contract(built, args):
    fs, f0, bw, lanes, D, L, gain = args
    margin = spec.rounding_margin(*args)
    assert margin > MARGIN, "an unrounded tap of this case sits on a rounding boundary (%.3g): pick another" % margin
    taps, shift, info = built._native.decim_design(fs, f0, bw, lanes, D, L, gain)
    want, want_shift, fs_out, f_out, inverted = spec.design(*args)
    assert shift == want_shift == spec.DESIGN_SHIFT
    assert taps.dtype == np.int16 and taps.size == lanes * L and np.array_equal(taps, want)
    assert (info["fs_out"], info["f_out"], info["inverted"]) == (fs_out, f_out, inverted)       # exactly
    spec.check(taps, shift, lanes, D)                                          # what it designs, the decimator takes


def test_where_the_band_lands(built):
    """The numbers of the three front ends the stage was specified on, zones 0 .. 5 of a real record with their inversion,
    and the I/Q wrap on both sides."""
    n = built._native
    _, _, a = n.decim_design(38192000.0, 9548000.0, 2046000.0, 1, 5)
    assert (a["fs_out"], a["inverted"]) == (7638400.0, False) and abs(a["f_out"] - 1909600.0) < 1e-6
    _, _, a = n.decim_design(38192000.0, 9548000.0, 2046000.0, 1, 3)
    assert a["inverted"] is True and abs(a["fs_out"] - 38192000.0 / 3) < 1e-6 and abs(a["f_out"] - 3182666.6667) < 1e-3
    _, _, a = n.decim_design(16368000.0, 3200000.0, 2046000.0, 2, 4)
    assert (a["fs_out"], a["inverted"]) == (4092000.0, False) and abs(a["f_out"] + 892000.0) < 1e-6
    seen = set()
    for args in GRID:
        fs, f0, bw, lanes, D, L, gain = args
        fo, f_out, inv = spec.output_settings(fs, f0, bw, lanes, D)
        if lanes == 1:
            z = int(f0 // (fo / 2))
            seen.add(z)
            assert inv == bool(z & 1) and 0 < f_out < fo / 2
            assert abs((fo / 2 - f_out if inv else f_out) - (f0 - z * fo / 2)) < 1e-6
        else:
            assert not inv and -fo / 2 <= f_out < fo / 2 and abs((f0 - f_out) / fo - round((f0 - f_out) / fo)) < 1e-9
            seen.add("up" if f_out < f0 else ("down" if f_out > f0 else "stay"))
    assert seen >= {0, 1, 2, 3, 4, 5, "up", "down", "stay"}


def _design_rc(n, fs=38192000.0, f0=9548000.0, bw=2046000.0, lanes=1, D=5, L=127, gain=0.0, null=None):
    taps = np.zeros(1100, dtype=np.int16)
    shift, inv, fo, f = C.c_int32(0), C.c_int32(0), C.c_double(0), C.c_double(0)
    ptrs = dict(taps=n._ptr(taps), shift=C.byref(shift), fs_out=C.byref(fo), f_out=C.byref(f), inverted=C.byref(inv))
    if null:
        ptrs[null] = None
    return n.lib().sgx_decim_design(fs, f0, bw, lanes, D, L, gain, ptrs["taps"], ptrs["shift"], ptrs["fs_out"],
                                    ptrs["f_out"], ptrs["inverted"])


def test_design_refusals(built):
    n = built._native
    assert _design_rc(n) == n.SGX_OK

    def refused(word, contract=True, **kw):
        assert _design_rc(n, **kw) == n.SGX_E_ARG and word in n.last_error(), (kw, n.last_error())
        if contract:
            a = dict(fs=38192000.0, f0=9548000.0, bw=2046000.0, lanes=1, D=5, L=127, gain=0.0)
            a.update(kw)
            with pytest.raises(ValueError):
                spec.design(a["fs"], a["f0"], a["bw"], a["lanes"], a["D"], a["L"], a["gain"])

    for name in ("taps", "shift", "fs_out", "f_out", "inverted"):
        refused(name, contract=False, null=name)
    for fs in (0.0, -1.0, np.inf, np.nan):
        refused("fs", fs=fs)
    for bw in (0.0, -2e6, np.inf, np.nan):
        refused("bandwidth_hz", bw=bw)
    refused("f0", f0=np.nan)
    refused("gain", gain=np.inf)
    for lanes in (0, 3):
        refused("lanes", lanes=lanes)
    for D in (0, 1, 17, -4):
        refused("D", D=D)
    for L in (0, 2, 126, 513, -1):
        refused("n_taps", L=L)
    # a band that aliases onto itself: the default record at D = 2 and 4 (its IF on a zone edge) is named
    for D in (2, 4):
        refused("zone", D=D)
        assert "38.192 Msps" in n.last_error() and "9.548 MHz" in n.last_error()
    refused("zone", fs=40000000.0, f0=2400000.0, D=8)            # 1.377 .. 3.423 MHz straddles 2.5 MHz
    refused("zone", fs=40000000.0, f0=-3000000.0, D=8)           # a real record has no negative IF
    refused("zone", fs=40000000.0, f0=21000000.0, D=8)           # beyond the input's Nyquist frequency
    refused("zone", fs=40000000.0, f0=1000000.0, D=8)            # 0 is an edge too: the band must clear it
    refused("bandwidth_hz", lanes=2, fs=16368000.0, f0=0.0, D=8)          # 2.046 MHz at 2.046 Msps
    refused("bandwidth_hz", lanes=2, fs=16368000.0, f0=0.0, D=4, bw=4092000.0)
    # a tap beyond what the decimator takes
    refused("32512", gain=40.0)
    refused("32512", lanes=2, fs=16368000.0, f0=0.0, D=4, gain=1000.0)
    assert n.lib().sgx_decim_timing(None, None) == n.SGX_E_ARG
    assert n.lib().sgx_decim_tile(None) == n.SGX_E_ARG
    assert n.decim_tile() > 0 and n.decim_tile() % 16 == 0


# ---- the decimator's refusals that need no record -----------------------------------------------------------------------

def _decimate_rc(n, taps, n_taps=None, shift=14, lanes=1, D=4, flags=0, null_taps=False):
    h = np.ascontiguousarray(taps, dtype=np.int16)
    out = C.c_void_p()
    return n.lib().sgx_if_decimate(None, None, lanes, None if null_taps else n._ptr(h),
                                   h.size // lanes if n_taps is None else n_taps, shift, D, flags, C.byref(out), None)


def test_decimator_refuses_bad_arguments_before_it_looks_at_the_device(built):
    """Every precondition of the contract that needs no record: each refusal is SGX_E_ARG and names its own argument (and
    the contract's check() raises on it); good arguments get as far as the missing context."""
    n = built._native
    good = np.arange(-31, 32, dtype=np.int16)
    far = "c && rec && out"
    for lanes, h in ((1, good), (2, np.tile(good, 2))):
        assert _decimate_rc(n, h, lanes=lanes) == n.SGX_E_ARG and far in n.last_error()
        assert _decimate_rc(n, h, lanes=lanes, flags=spec.OFFSET_BINARY) == n.SGX_E_ARG and far in n.last_error()
        spec.check(h, 14, lanes, 4, spec.OFFSET_BINARY)
    for lanes in (0, 3, -1):
        assert _decimate_rc(n, good, lanes=lanes, n_taps=63) == n.SGX_E_ARG and "lanes" in n.last_error()
        with pytest.raises(ValueError):
            spec.check(good, 14, lanes, 4)
    for D in (-2, 0, 1, 17, 32):
        assert _decimate_rc(n, good, D=D) == n.SGX_E_ARG and "D = %d" % D in n.last_error()
        with pytest.raises(ValueError):
            spec.check(good, 14, 1, D)
    for D in range(2, 17):
        assert _decimate_rc(n, good, D=D) == n.SGX_E_ARG and far in n.last_error()
    for L in (0, 2, 62, 512, 513, -1):
        assert _decimate_rc(n, np.zeros(1100, dtype=np.int16), n_taps=L) == n.SGX_E_ARG and "n_taps" in n.last_error(), L
        if L > 0:
            with pytest.raises(ValueError):
                spec.check(np.zeros(L, dtype=np.int16), 14, 1, 4)
    assert _decimate_rc(n, np.zeros(511, dtype=np.int16)) == n.SGX_E_ARG and far in n.last_error()
    for shift in (-1, 31):
        assert _decimate_rc(n, good, shift=shift) == n.SGX_E_ARG and "shift" in n.last_error()
        with pytest.raises(ValueError):
            spec.check(good, shift, 1, 4)
    for flags in (2, 4, 3, -1, 1 << 30):
        assert _decimate_rc(n, good, flags=flags) == n.SGX_E_ARG and "flags" in n.last_error(), flags
        with pytest.raises(ValueError):
            spec.check(good, 14, 1, 4, flags)
    assert _decimate_rc(n, good, null_taps=True) == n.SGX_E_ARG and "taps" in n.last_error()
    for lanes in (1, 2):
        for at in (3, 4):                                                      # a real part and an imaginary one
            for v in (32513, -32513, 32767, -32768):
                big = np.tile(good, lanes)
                big[at] = v
                assert _decimate_rc(n, big, lanes=lanes) == n.SGX_E_ARG and "32512" in n.last_error(), v
                with pytest.raises(ValueError):
                    spec.check(big, 14, lanes, 4)
            for v in (32512, -32512):
                big = np.tile(good, lanes)
                big[at] = v
                assert _decimate_rc(n, big, lanes=lanes) == n.SGX_E_ARG and far in n.last_error(), v
    # 128 sum|h| < 2^31: out of reach of 511 real taps of at most 32 512, within reach of 511 complex ones, where the sum is
    # that of |re| + |im|
    full = np.full(511, 32512, dtype=np.int16)
    assert 128 * int(np.abs(full.astype(np.int64)).sum()) < 2 ** 31
    assert _decimate_rc(n, full) == n.SGX_E_ARG and far in n.last_error()
    budget = (2 ** 31 - 1) // 128
    cplx = np.zeros(1022, dtype=np.int16)
    cplx[:budget // 32512] = 32512
    cplx[budget // 32512] = budget - 32512 * (budget // 32512)
    assert 128 * int(np.abs(cplx.astype(np.int64)).sum()) == 2 ** 31 - 128
    assert _decimate_rc(n, cplx, lanes=2) == n.SGX_E_ARG and far in n.last_error()
    spec.check(cplx, 0, 2, 4)
    cplx[-1] = 1                                                               # one more LSB, in an imaginary part
    assert _decimate_rc(n, cplx, lanes=2) == n.SGX_E_ARG and "2^31" in n.last_error()
    with pytest.raises(ValueError):
        spec.check(cplx, 0, 2, 4)
    with pytest.raises(ValueError):
        spec.check(np.tile(good, 2), 14, 2, 4, 0, n_bytes=7)
    spec.check(good, 14, 1, 4, 0, n_bytes=7)


# ---- the contract's own properties --------------------------------------------------------------------------------------

def test_the_two_forms_of_the_contract_agree():
    """decim_spec sums phase by phase for speed; the sums as the contract writes them, tap by tap, are the same."""
    rng = np.random.default_rng(21)
    for D in (2, 3, 5, 16):
        for L in (1, 3, 2 * D - 1, 2 * D + 1, 63, 511):
            for N in (0, 1, D - 1, D, D + 1, L, 1000, 1001):
                x = rng.integers(-128, 128, N).astype(np.int64)
                h = rng.integers(-3000, 3000, L).astype(np.int64)
                n_out = -(-N // D)
                assert np.array_equal(spec._fir_at(x, h, D, n_out), spec.fir_direct(x, h, D, n_out)), (D, L, N)


def test_contract_closed_forms():
    rng = np.random.default_rng(22)
    b = rng.integers(-128, 128, 4001).astype(np.int8)
    one = np.array([1], dtype=np.int16)
    for D in (2, 3, 16):
        y, clipped = spec.decimate(b, one, 0, 1, D)                            # [1]: every D-th sample, -128 clipped
        assert np.array_equal(y, np.clip(b[::D].astype(np.int64), -127, 127)) and clipped == np.count_nonzero(b[::D] == -128)
        assert y.size == -(-b.size // D)
        # h[c + 1] alone is a delay of one input sample; the first output sees the zero in front of the record
        y, _ = spec.decimate(b, np.array([0, 0, 1], dtype=np.int16), 0, 1, D)
        assert y[0] == 0 and np.array_equal(y[1:], np.clip(b[D - 1::D].astype(np.int64), -127, 127)[:y.size - 1])
    # j: (I + jQ) j = -Q + jI
    y, _ = spec.decimate(b[:4000], np.array([0, 1], dtype=np.int16), 0, 2, 4)
    I, Q = b[0:4000:8].astype(np.int64), b[1:4000:8].astype(np.int64)
    assert np.array_equal(y[0::2], np.clip(-Q, -127, 127)) and np.array_equal(y[1::2], np.clip(I, -127, 127))
    # rounding: half up before the floor shift; offset binary is byte - 128
    y, _ = spec.decimate(np.array([1, 3, -1, -3], dtype=np.int8), one, 1, 1, 2)
    assert list(y) == [1, 0]
    u8 = b.view(np.uint8) ^ 0x80
    h = rng.integers(-300, 301, 31).astype(np.int16)
    assert np.array_equal(spec.decimate(u8, h, 7, 1, 3, spec.OFFSET_BINARY)[0], spec.decimate(b, h, 7, 1, 3)[0])


def test_q_first_identity():
    """Filtering Q + jI with conj(h) gives Im w + j Re w: a Q-first file through the conjugated taps is the I-first file's
    output with its bytes swapped - Q-first again - clip count and all."""
    rng = np.random.default_rng(23)
    b = rng.integers(-128, 128, 6000).astype(np.int8)
    swapped = b.reshape(-1, 2)[:, ::-1].ravel()
    for D, L, S in ((4, 63, 14), (3, 5, 0), (16, 127, 11)):
        h = rng.integers(-2000, 2001, 2 * L).astype(np.int16)
        conj = h.copy()
        conj[1::2] = -conj[1::2]
        y, c = spec.decimate(b, h, S, 2, D)
        yq, cq = spec.decimate(swapped, conj, S, 2, D)
        assert np.array_equal(yq.reshape(-1, 2)[:, ::-1].ravel(), y) and cq == c


def _tone(lanes, f_rel, frames, amp=100.0):
    t = np.arange(frames)
    if lanes == 1:
        return np.rint(amp * np.cos(2 * np.pi * f_rel * t + 0.4)).astype(np.int8)
    z = amp * np.exp(1j * (2 * np.pi * f_rel * t + 0.4))
    b = np.empty(2 * frames, dtype=np.int8)
    b[0::2], b[1::2] = np.rint(z.real), np.rint(z.imag)
    return b


def _spectrum(y, lanes):
    """(frequencies in cycles per output sample, power) of a decimated record under a Blackman-Harris window."""
    z = y.astype(np.float64)
    z = z[0::2] + 1j * z[1::2] if lanes == 2 else z
    n = z.size
    k = np.arange(n)
    w = (0.35875 - 0.48829 * np.cos(2 * np.pi * k / n) + 0.14128 * np.cos(4 * np.pi * k / n)
         - 0.01168 * np.cos(6 * np.pi * k / n))
    return np.fft.fftfreq(n), np.abs(np.fft.fft(z * w)) ** 2


@pytest.mark.parametrize("args", [g for g in GRID if g[5] >= 63], ids=lambda g: "%g-%g-%d-D%d-L%d" % (g[0] / 1e6, g[1] / 1e6,
                                                                                                       g[3], g[4], g[5]))
def test_a_tone_in_the_band_comes_out_at_f_out(args):
    """A tone 150 kHz above the carrier comes out 150 kHz above f_out - below it where the band is inverted."""
    fs, f0, bw, lanes, D, L, gain = args
    h, S, fo, f_out, inv = spec.design(fs, f0, bw, lanes, D, L, 1.0)
    df = 150e3
    y, clipped = spec.decimate(_tone(lanes, (f0 + df) / fs, 8192 * D), h, S, lanes, D)
    assert clipped == 0
    f, p = _spectrum(y, lanes)
    peak = f[int(np.argmax(p))] * fo
    want = f_out + (-df if inv else df)
    assert abs(abs(peak) - abs(want)) < 2 * fo / (8192.0) and (lanes == 1 or peak * want > 0), (peak, want)
    # ... at the amplitude it had: the design's gain of 1 in the band
    amp = np.sqrt(2.0 * np.mean(y.astype(np.float64) ** 2))    # (a sinusoid's rms, and each component's of a complex tone)
    assert 90.0 < amp < 110.0, amp


def alias_rejection_db(fs, f0, lanes, D, L=spec.DEFAULT_TAPS):
    """The weakest rejection of a full-scale tone that would alias into the kept band: for every frequency of the output
    band f_out +- 0.4 bandwidth, every input frequency other than the wanted one that lands there, against the wanted one
    itself."""
    bw = spec.DEFAULT_BANDWIDTH
    h, S, fo, f_out, inv = spec.design(fs, f0, bw, lanes, D, L, 1.0)
    frames = 4096 * D

    def power(f_in):
        y, _ = spec.decimate(_tone(lanes, f_in / fs, frames), h, S, lanes, D)
        return float(np.sum(y.astype(np.float64) ** 2))

    worst = np.inf
    for off in (-0.4 * bw, -0.13 * bw, 0.27 * bw, 0.4 * bw):
        wanted = power(f0 + off)
        images = []
        if lanes == 2:
            images = [f0 + off + k * fo for k in range(-D, D + 1) if k and abs(f0 + off + k * fo) < fs / 2]
        else:
            base = (f0 + off) % fo
            images = [f for k in range(D + 1) for f in (k * fo + base, k * fo - base)
                      if 0 < f < fs / 2 and abs(f - (f0 + off)) > 1.0]
        for f_in in images:
            worst = min(worst, 10.0 * np.log10(wanted / max(power(f_in), 1e-12)))
    return worst


@pytest.mark.parametrize("D", sorted(ALIAS_REJECTION_DB))
def test_alias_rejection_of_the_default_design(D):
    if D in (3, 5):
        worst = alias_rejection_db(38192000.0, 9548000.0, 1, D)               # the default record
    else:
        worst = alias_rejection_db(16368000.0, 3200000.0, 2, D) if D == 4 else alias_rejection_db(40000000.0, 6200000.0, 1, D)
    print("alias rejection, %d taps, D = %d: %.2f dB" % (spec.DEFAULT_TAPS, D, worst))
    assert worst >= ALIAS_REJECTION_DB[D] - 3.0, worst


# ---- the Settings surface -----------------------------------------------------------------------------------------------

def test_settings_surface(built):
    s = built.Settings()
    assert (s.decimation, s.decimTaps, s.decimBandwidth, s.decimGain) == (0, 127, 2.046e6, 0.0)
    assert s._prepared_settings() is s                                         # off: a plain record is read as it is
    with pytest.raises(ValueError, match="decimation"):
        s.decimateRecord(None)
    s.decimation = 5
    real = s._prepared_settings()
    assert real is not s and (real.samplingFreq, real.decimation, real.dataType) == (7638400.0, 0, 'int8')
    assert abs(real.IF - 1909600.0) < 1e-6 and real.samplesPerCode == 7638
    assert (s.samplingFreq, s.IF, s.decimation) == (38192000.0, 9548000.0, 5)  # left alone
    assert s._decim_format() == (1, 5, 127, False, False)
    taps, shift, info = s._decim_design()
    want = spec.design(38192000.0, 9548000.0, 2.046e6, 1, 5, 127)
    assert np.array_equal(taps, want[0]) and shift == want[1] and (info["fs_out"], info["f_out"], info["inverted"]) == want[2:]
    s.decimation = 3
    assert s._prepared_settings().samplesPerCode == 12731 and s._decim_design()[2]["inverted"] is True
    # every refused combination names its setting
    for D in (1, 17, -2, 2.5, "x"):
        s.decimation = D
        with pytest.raises(ValueError, match="decimation"):
            s.postProcessing("/nonexistent/record.bin")
    for D in (2, 4):                                                           # the default record's IF on a zone edge
        s.decimation = D
        with pytest.raises(ValueError, match="zone"):
            s.postProcessing("/nonexistent/record.bin")
    s.decimation = 5
    for L in (0, 2, 513, 63.5):
        s.decimTaps = L
        with pytest.raises(ValueError, match="decimTaps"):
            s.postProcessing("/nonexistent/record.bin")
    s.decimTaps = 127
    for bw in (0.0, -1.0, 4e6):
        s.decimBandwidth = bw
        with pytest.raises(ValueError, match="decimBandwidth"):
            s.postProcessing("/nonexistent/record.bin")
    s.decimBandwidth = 2.046e6
    s.decimGain = 1e4
    with pytest.raises(ValueError, match="decimGain"):
        s.postProcessing("/nonexistent/record.bin")
    s.decimGain = 0.0
    for dt in ('uint8', 'int16', 'float32', 'float64'):                        # a real record is int8 where the stage sees it
        s.dataType = dt
        with pytest.raises(ValueError, match="dataType"):
            s.postProcessing("/nonexistent/record.bin")
    # ... which the conditioning stage and the unpacker see to
    s.frontEndConditioning = True
    for dt in ('uint8', 'int16', 'int8'):
        s.dataType = dt
        real = s._prepared_settings()
        assert (real.dataType, real.frontEndConditioning, real.decimation, real.samplingFreq) == ('int8', False, 0, 7638400.0)
    s.dataType = 'float32'
    with pytest.raises(ValueError, match="float32"):
        s._prepared_settings()
    s.frontEndConditioning, s.dataType, s.packedBits = False, 'int8', 2
    real = s._prepared_settings()
    assert (real.packedBits, real.decimation, real.samplingFreq) == (0, 0, 7638400.0)
    s.packedBits = 0
    # I/Q: whatever reaches the converter today; uint8 goes through the stage's offset-binary flag, Q first through
    # conjugated taps, and the converter is told int8
    s.iqRecord, s.samplingFreq, s.IF, s.decimation, s.decimTaps = True, 16368000.0, 3200000.0, 4, 63
    assert s._decim_format() == (2, 4, 63, False, False)
    real = s._prepared_settings()
    assert (real.samplingFreq, real.IF, real.iqRecord, real.dataType, real.decimation) == (8184000.0, 1154000.0, False, 'int8', 0)
    s.dataType, s.iqQFirst = 'uint8', True
    assert s._decim_format() == (2, 4, 63, True, True)
    front = s._walk(upto="convert")[1]
    assert (front.dataType, front.iqRecord, front.iqQFirst, front.samplingFreq, front.IF) == ('int8', True, True, 4092000.0,
                                                                                              -892000.0)
    assert front._iq_format() == (True, False)
    taps = s._decim_design()[0]
    want = spec.design(16368000.0, 3200000.0, 2.046e6, 2, 4, 63)[0]
    assert np.array_equal(taps[0::2], want[0::2]) and np.array_equal(taps[1::2], -want[1::2])
    s.dataType = 'int16'
    with pytest.raises(ValueError, match="int8"):
        s._prepared_settings()
    s.iqRequantize = True
    assert s._decim_format() == (2, 4, 63, False, True)
    assert s._prepared_settings().samplingFreq == 8184000.0
    s.decimation = 8                                                           # 2.046 MHz do not fit 2.046 Msps
    with pytest.raises(ValueError, match="decimBandwidth"):
        s._prepared_settings()


def test_skip_arithmetic(built):
    """skipNumberOfBytes is a byte of the file on a multiple of D frames; it becomes that frame / D of the decimated record,
    in bytes of the prepared record."""
    for lanes, fs, f0, dt, w in ((1, 38192000.0, 9548000.0, 'int8', 1), (2, 16368000.0, 3200000.0, 'int8', 1),
                                 (2, 16368000.0, 3200000.0, 'uint8', 1), (2, 16368000.0, 3200000.0, 'int16', 2),
                                 (2, 16368000.0, 3200000.0, 'float32', 4), (1, 38192000.0, 9548000.0, 'int16', 2)):
        for D in (3, 5) if lanes == 1 else (2, 3, 4, 7):
            s = built.Settings()
            s.samplingFreq, s.IF, s.iqRecord, s.dataType, s.decimation = fs, f0, lanes == 2, dt, D
            s.iqRequantize = lanes == 2 and w > 1
            s.frontEndConditioning = lanes == 1 and w > 1
            unit = w * lanes * D
            for k in (0, 1, 5, 1237):
                s.skipNumberOfBytes = k * unit
                real = s._prepared_settings()
                assert real.skipNumberOfBytes == k * lanes, (lanes, dt, D, k)
                assert abs(real.samplingFreq - lanes * fs / D) < 1e-6 and not real.iqRecord and real.dataType == 'int8'
                assert s.skipNumberOfBytes == k * unit
            for skip in (1, unit - 1, unit + 1, 3 * unit + unit // 2, w * lanes, w * lanes * (D - 1)):
                if skip % unit:
                    s.skipNumberOfBytes = skip
                    with pytest.raises(ValueError, match="skipNumberOfBytes = %d" % skip):
                        s._prepared_settings()
                    with pytest.raises(ValueError, match="skipNumberOfBytes = %d" % skip):
                        s.postProcessing("/nonexistent/record.bin")
    # behind the unpacker: a byte of the packed file, on a frame of the packed file that starts a group of D samples
    s = built.Settings()
    s.packedBits, s.decimation = 2, 5
    s.skipNumberOfBytes = 5 * 7
    assert s._prepared_settings().skipNumberOfBytes == 4 * 7
    s.skipNumberOfBytes = 6
    with pytest.raises(ValueError, match="skipNumberOfBytes"):
        s._prepared_settings()
    for case in cases.CASES.values():
        s = case.settings(built, skipNumberOfBytes=case.D * case.lanes * cases.SKIP_GROUPS)
        assert s._prepared_settings().skipNumberOfBytes == case.lanes * cases.SKIP_GROUPS
        real = s._prepared_settings()
        assert (real.samplingFreq, real.IF) == case.prepared_rate()


# ---- the scenes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_scenes_are_well_conditioned(name):
    """The contracts' record under the oracle's search: exactly the scene's satellites, where the scene put them - an
    inverted band shows the Doppler with the other sign - and every one of the 28 absent PRNs at or below ABSENT_MAX: the
    precondition of the end-to-end tests on the GPU."""
    case = cases.CASES[name]
    scene = case.scene
    o = case.oracle_settings()
    assert (o.samplingFreq, o.IF) == case.prepared_rate()
    y = cases.prepared(case, cases.ACQ_MS)
    assert y.size == -(-cases.ACQ_MS * scene.frames_per_ms // case.D) * case.lanes
    a = np.abs(y.astype(np.int64))
    win = np.concatenate(([0], np.cumsum(a)))
    _, clipped = spec.decimate(cases.file_of(case, cases.ACQ_MS), case.taps, case.shift, case.lanes, case.D)
    print("%s: rms %.2f, max |y| %d, %d clipped, largest 2048-sample sum of magnitudes %d"
          % (name, float(np.sqrt(np.mean(y.astype(np.float64) ** 2))), a.max(), clipped, (win[2048:] - win[:-2048]).max()))
    assert (win[2048:] - win[:-2048]).max() < 131072                           # tracking stays on its fastest kernel
    n = o.samplesPerCode
    for groups in (0, cases.SKIP_GROUPS):                                      # the two windows the GPU tests acquire in
        ref = cases.contract_acquisition(case, groups)
        assert sorted(np.flatnonzero(ref["carrFreq"]) + 1) == sorted(scene.prns)
        absent = [p for p in range(1, 33) if p not in scene.prns]
        assert len(absent) == 28
        others = np.asarray(ref["peakMetric"])[[p - 1 for p in absent]]
        print("%s, skip %d: largest peak metric among the 28 absent PRNs %.3f" % (name, groups, float(others.max())))
        assert others.max() <= cases.ABSENT_MAX
        for i, prn in enumerate(scene.prns):
            f, c, pm = ref["carrFreq"][prn - 1], ref["codePhase"][prn - 1], ref["peakMetric"][prn - 1]
            off = (c - (case.true_phase(i) - groups * case.lanes) + n / 2.0) % n - n / 2.0
            print("%s, skip %d, PRN %2d: carrFreq %+.1f Hz, code phase %+.2f samples off the truth, peak metric %.1f"
                  % (name, groups, prn, f - case.true_carrier(i), off, pm))
            assert abs(f - case.true_carrier(i)) <= cases.CARR_TOL_HZ
            assert abs(off) <= cases.PHASE_TOL
            assert pm >= cases.MARGIN * o.acqThreshold
