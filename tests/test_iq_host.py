"""CPU-only checks of the I/Q front stage (include/sgx.h: sgx_iq_design, and the argument refusals of sgx_if_from_iq that
need no device) against the numpy contract of tests/iq_spec.py; the contract's own properties - the closed forms of the
shortest filters, the flags, the image rejection of the designed filter; the two scenes of tests/iq_cases.py shown to be
well conditioned by the contract plus the oracle alone; and the Settings surface."""
import ctypes as C
import importlib

import numpy as np
import pytest

import iq_cases as cases
import iq_spec as spec
from conftest import pkg

MARGIN = 1e-6
# Image rejection of the 63-tap design, measured on the contract with full-scale tones at |f| <= 0.4 fs_c: 60.3 dB (the
# worst tone is the one at the band edge, +-0.4 fs_c); 3 dB are taken off for the placement of a tone between two bins.
IMAGE_REJECTION_63_DB = 60.3


@pytest.fixture(scope="module")
def built():
    importlib.import_module("__graft_entry__").build()
    return pkg()


@pytest.mark.parametrize("L", [1, 3, 31, 63, 255])
def test_design_equals_the_contract(built, L):
    taps, shift = built._native.iq_design(L)
    want, want_shift = spec.design(L)
    assert shift == want_shift == spec.DESIGN_SHIFT
    assert taps.dtype == np.int16 and np.array_equal(taps, want)


@pytest.mark.parametrize("L", [1, 3, 31, 63, 255])
def test_designed_taps_are_a_half_band_filter(built, L):
    taps, shift = built._native.iq_design(L)
    c = (L - 1) // 2
    m = np.arange(L) - c
    assert taps[c] == 1 << shift == 16384
    assert not np.any(taps[(m % 2 == 0) & (m != 0)])
    assert np.array_equal(taps, taps[::-1])
    spec.check(taps, shift)
    if L >= 31:                                      # the odd-m taps carry the other half of the gain of 2
        assert abs(int(taps.astype(np.int64).sum()) - 2 * 16384) <= 16384 // 50


def test_default_length_keeps_clear_of_rounding_boundaries(built):
    assert built.Settings().iqTaps == spec.DEFAULT_TAPS
    margin = spec.rounding_margin(spec.DEFAULT_TAPS)
    assert margin > MARGIN, "a tap of the default design sits on a rounding boundary (%.3g)" % margin


def test_design_refusals(built):
    n = built._native
    taps = np.zeros(512, dtype=np.int16)
    shift = C.c_int32(0)
    assert n.lib().sgx_iq_design(63, n._ptr(taps), C.byref(shift)) == n.SGX_OK
    for L in (0, -1, 2, 62, 256, 257, 4095):
        assert n.lib().sgx_iq_design(L, n._ptr(taps), C.byref(shift)) == n.SGX_E_ARG, L
    assert n.lib().sgx_iq_design(63, None, C.byref(shift)) == n.SGX_E_ARG
    assert n.lib().sgx_iq_design(63, n._ptr(taps), None) == n.SGX_E_ARG
    assert n.lib().sgx_iq_timing(None, None) == n.SGX_E_ARG
    assert n.lib().sgx_iq_tile(None) == n.SGX_E_ARG
    assert n.iq_tile() > 0 and n.iq_tile() % 16 == 0


def _convert_rc(n, taps, shift, flags=0, n_taps=None, null_taps=False):
    h = np.ascontiguousarray(taps, dtype=np.int16)
    out = C.c_void_p()
    return n.lib().sgx_if_from_iq(None, None, None if null_taps else n._ptr(h), h.size if n_taps is None else n_taps,
                                  shift, flags, C.byref(out))


def test_converter_refuses_bad_arguments_before_it_looks_at_the_device(built):
    """Every precondition of the contract that needs no record: each refusal is SGX_E_ARG and names its own condition (and
    the contract's check() raises on it); good arguments get as far as the missing context."""
    n = built._native
    good, S = spec.design(63)
    assert _convert_rc(n, good, S) == n.SGX_E_ARG and "c && iq_bytes && out" in n.last_error()
    for flags in (1, 2, 3):
        assert _convert_rc(n, good, S, flags) == n.SGX_E_ARG and "c && iq_bytes && out" in n.last_error()
    assert _convert_rc(n, good, S, null_taps=True) == n.SGX_E_ARG and "taps" in n.last_error()
    for L in (0, 2, 62, 256, 257):
        assert _convert_rc(n, np.zeros(300, dtype=np.int16), S, n_taps=L) == n.SGX_E_ARG
        assert "n_taps" in n.last_error(), L
        if L:
            with pytest.raises(ValueError):
                spec.check(np.zeros(L, dtype=np.int16), S)
    for shift in (-1, 31):
        assert _convert_rc(n, good, shift) == n.SGX_E_ARG and "shift" in n.last_error()
        with pytest.raises(ValueError):
            spec.check(good, shift)
    for flags in (4, 8, 7, -1, 1 << 30):
        assert _convert_rc(n, good, S, flags) == n.SGX_E_ARG and "flags" in n.last_error(), flags
        with pytest.raises(ValueError):
            spec.check(good, S, flags)
    for v in (32513, -32513, 32767, -32768):
        big = good.copy()
        big[3] = v
        assert _convert_rc(n, big, S) == n.SGX_E_ARG and "32512" in n.last_error(), v
        with pytest.raises(ValueError):
            spec.check(big, S)
    for v in (32512, -32512):
        big = good.copy()
        big[3] = v
        assert _convert_rc(n, big, S) == n.SGX_E_ARG and "c && iq_bytes && out" in n.last_error(), v
    # 128 sum|h| < 2^31 cannot fail within 255 taps of at most 32 512 (255 * 32 512 < 2^24): the bound is the contract's
    # all the same, and the largest admitted filter passes it
    full = np.full(255, 32512, dtype=np.int16)
    assert 128 * int(np.abs(full.astype(np.int64)).sum()) < 2 ** 31
    assert _convert_rc(n, full, 0) == n.SGX_E_ARG and "c && iq_bytes && out" in n.last_error()
    with pytest.raises(ValueError):
        spec.check(good, S, 0, n_bytes=7)


def test_contract_closed_forms():
    """The shortest filters, where the contract can be written down by hand.  [1]: zero-stuffing leaves the half-period
    instants empty, y = I, 0, -I, 0.  [0, 1, 1] holds each pair for both its instants: y = I, -Q, -I, Q."""
    rng = np.random.default_rng(11)
    b = rng.integers(-127, 128, 4000).astype(np.int8)
    I, Q = b[0::2].astype(np.int64), b[1::2].astype(np.int64)
    sign = np.where(np.arange(I.size) % 2 == 0, 1, -1)
    y = spec.convert(b, np.array([1], dtype=np.int16), 0)
    assert np.array_equal(y[0::2], sign * I) and not y[1::2].any()
    y = spec.convert(b, np.array([0, 1, 1], dtype=np.int16), 0)
    assert np.array_equal(y[0::2], sign * I) and np.array_equal(y[1::2], -sign * Q)
    # h[c + 1] alone is the half-period delay: the odd instants see the pair before them
    y = spec.convert(b, np.array([0, 0, 1], dtype=np.int16), 0)
    assert not y[0::2].any() and np.array_equal(y[1::2], -sign * Q)
    # h[c - 1] alone: the odd instants see the pair AFTER them, the last one the zero beyond the record
    y = spec.convert(b, np.array([1, 0, 0], dtype=np.int16), 0)
    assert np.array_equal(y[1:-1:2], (-sign * np.roll(Q, -1))[:-1]) and y[-1] == 0
    # -128 is legal input and leaves through the clip as -127 or +127
    e = np.array([-128, -128, -128, -128], dtype=np.int8)
    assert list(spec.convert(e, np.array([0, 1, 1], dtype=np.int16), 0)) == [-127, 127, 127, -127]


def test_contract_flags():
    rng = np.random.default_rng(12)
    b = rng.integers(-128, 128, 3000).astype(np.int8)
    h = rng.integers(-300, 301, 31).astype(np.int16)
    y = spec.convert(b, h, 7)
    swapped = b.reshape(-1, 2)[:, ::-1].ravel()
    assert np.array_equal(spec.convert(swapped, h, 7, spec.Q_FIRST), y)
    u8 = (b.view(np.uint8) ^ 0x80)
    assert np.array_equal(u8.astype(np.int64) - 128, (u8 ^ 0x80).view(np.int8).astype(np.int64))
    assert np.array_equal(spec.convert(u8, h, 7, spec.OFFSET_BINARY), y)
    assert np.array_equal(spec.convert(u8.reshape(-1, 2)[:, ::-1].ravel(), h, 7, spec.OFFSET_BINARY | spec.Q_FIRST), y)


def image_rejection_db(L, f_rel, pairs=8192):
    """A full-scale complex tone at f_rel fs_c through the contract: its power at fs_c / 2 + f over the power at the image
    fs_c / 2 - f, each summed over +-4 bins of a Blackman-Harris window."""
    h, S = spec.design(L)
    z = 127.0 * np.exp(2j * np.pi * f_rel * np.arange(pairs))
    b = np.empty(2 * pairs, dtype=np.int8)
    b[0::2] = np.rint(z.real)
    b[1::2] = np.rint(z.imag)
    y = spec.convert(b, h, S).astype(np.float64)
    n = y.size
    k = np.arange(n)
    w = (0.35875 - 0.48829 * np.cos(2 * np.pi * k / n) + 0.14128 * np.cos(4 * np.pi * k / n)
         - 0.01168 * np.cos(6 * np.pi * k / n))
    p = np.abs(np.fft.rfft(y * w)) ** 2

    def band(f_out):                                 # cycles per OUTPUT sample
        c = int(round(f_out * n))
        return p[max(c - 4, 0):c + 5].sum()

    return 10.0 * np.log10(band(0.25 + f_rel / 2.0) / band(0.25 - f_rel / 2.0))


def test_image_rejection_of_the_default_design():
    tones = [sgn * f for f in [k / 40.0 + 0.0013 for k in range(1, 16)] + [0.4] for sgn in (1, -1)]
    worst = min(image_rejection_db(spec.DEFAULT_TAPS, f) for f in tones)
    print("image rejection, %d taps, |f| <= 0.4 fs_c: %.2f dB" % (spec.DEFAULT_TAPS, worst))
    assert worst >= IMAGE_REJECTION_63_DB - 3.0, worst


@pytest.mark.parametrize("scene", cases.SCENES, ids=[s.name for s in cases.SCENES])
def test_scenes_are_well_conditioned(scene):
    """The contract's record under the oracle's search: exactly the scene's satellites, where the scene put them."""
    ref = cases.contract_acquisition(scene)
    o = scene.oracle_settings()
    assert (o.samplingFreq, o.IF) == (2.0 * scene.fs_c, scene.f_bb + scene.fs_c / 2.0)
    assert sorted(np.flatnonzero(ref["carrFreq"]) + 1) == sorted(scene.prns)
    for i, prn in enumerate(scene.prns):
        f, c, pm = ref["carrFreq"][prn - 1], ref["codePhase"][prn - 1], ref["peakMetric"][prn - 1]
        print("%s PRN %2d: carrFreq %+.1f Hz, code phase %+.2f samples off the truth, peak metric %.1f"
              % (scene.name, prn, f - scene.true_carrier(i), c - scene.code_start[i], pm))
        assert abs(f - scene.true_carrier(i)) <= cases.CARR_TOL_HZ
        assert abs(c - scene.code_start[i]) <= cases.PHASE_TOL
        assert pm >= cases.MARGIN * o.acqThreshold


def test_settings_surface(built):
    s = built.Settings()
    assert (s.iqRecord, s.iqQFirst, s.iqTaps) == (False, False, 63)
    plain = s.realEquivalent()
    assert plain is not s and (plain.samplingFreq, plain.IF, plain.dataType) == (s.samplingFreq, s.IF, s.dataType)
    s.iqRecord, s.samplingFreq, s.IF, s.dataType = True, 4096000.0, -20000.0, 'uint8'
    real = s.realEquivalent()
    assert (real.samplingFreq, real.IF, real.iqRecord, real.dataType) == (8192000.0, 2028000.0, False, 'int8')
    assert (s.samplingFreq, s.IF, s.iqRecord, s.dataType) == (4096000.0, -20000.0, True, 'uint8')
    assert real.samplesPerCode == 8192 and real.iqTaps == 63
    assert s._iq_format() == (False, True)
    s.iqQFirst, s.dataType = True, 'int8'
    assert s._iq_format() == (True, False)
    for dt in ('int16', 'float32', 'uint16'):
        s.dataType = dt
        with pytest.raises(ValueError, match="int8"):
            s.postProcessing("/nonexistent/record.bin")
        with pytest.raises(ValueError, match="int8"):
            s.convertIQ(None)
    s.dataType, s.skipNumberOfBytes = 'int8', 3
    with pytest.raises(ValueError, match="even"):
        s.postProcessing("/nonexistent/record.bin")
