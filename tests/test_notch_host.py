"""CPU-only checks of the interference-excision stage's host code (include/sgx.h: sgx_notch_design, and the argument
refusals of sgx_if_filter that need no device) against the numpy contract of tests/notch_spec.py: line lists exactly
equal, taps exactly equal - every case is first shown to keep its unrounded taps 1e-9 away from a rounding boundary, so
an ulp of difference between two libraries' sin / cos cannot move a tap."""
import ctypes as C
import importlib

import numpy as np
import pytest

import notch_spec as spec
from conftest import pkg

N_BINS = 8193
FS = 38192000.0
MARGIN = 1e-9


@pytest.fixture(scope="module")
def built():
    importlib.import_module("__graft_entry__").build()
    return pkg()


def spectrum(lines, seed=1, n=N_BINS):
    """(f MHz, pxx): a gently sloped floor with +-1 dB of ripple and, per (bin, dB above the floor, bins wide) a line."""
    rng = np.random.default_rng(seed)
    f = np.fft.rfftfreq(2 * (n - 1), 1.0 / (FS / 1e6))
    pxx = (1.0 + 0.5 * np.arange(n) / n) * 10.0 ** (rng.uniform(-1.0, 1.0, n) / 10.0)
    for b, db, wide in lines:
        for k in range(wide):
            pxx[b + k] *= 10.0 ** ((db - 0.5 * abs(k - (wide - 1) / 2.0)) / 10.0)
    return f, pxx


NINE = [(400 + 800 * i, 14.0 + 3.0 * ((5 * i) % 9), 1) for i in range(9)]    # strengths all different; the weakest is i = 0
CASES = {
    "no line": ([], 8.0, 80e3, 1025),
    "one line": ([(2100, 30.0, 1)], 8.0, 80e3, 1025),
    "two lines, one of them wide": ([(1500, 25.0, 1), (5000, 40.0, 60)], 8.0, 80e3, 1025),
    "nine lines: the eight strongest are kept": (NINE, 8.0, 80e3, 1025),
    "a line at each band edge": ([(0, 30.0, 1), (N_BINS - 1, 30.0, 1)], 8.0, 80e3, 255),
    "flagged bins 3 apart are one line": ([(3000, 30.0, 1), (3003, 28.0, 1)], 8.0, 50e3, 4095),
    "flagged bins 4 apart are two lines": ([(3000, 30.0, 1), (3004, 28.0, 1)], 8.0, 50e3, 4095),
    "a higher threshold drops the weaker line": ([(1500, 12.0, 1), (5000, 30.0, 1)], 20.0, 120e3, 63),
    "a single tap": ([(2100, 30.0, 1)], 8.0, 80e3, 1),
}
EXPECTED_LINES = {"no line": 0, "one line": 1, "two lines, one of them wide": 2,
                  "nine lines: the eight strongest are kept": 8, "a line at each band edge": 2,
                  "flagged bins 3 apart are one line": 1, "flagged bins 4 apart are two lines": 2,
                  "a higher threshold drops the weaker line": 1, "a single tap": 1}


@pytest.mark.parametrize("name", sorted(CASES))
def test_design_equals_the_contract(built, name):
    lines_in, thr, width, L = CASES[name]
    f, pxx = spectrum(lines_in)
    s = built.Settings()
    want_lines = spec.detect(f, pxx, thr, width)
    assert len(want_lines) == EXPECTED_LINES[name], want_lines
    margin = spec.rounding_margin(want_lines, s.samplingFreq, L)
    assert margin > MARGIN, "the case sits on a rounding boundary (%.3g): choose another" % margin
    want_taps = spec.design(want_lines, s.samplingFreq, L)
    taps, shift, lines = built._native.notch_design(s, f, pxx, thr, width, L)
    assert lines == want_lines                       # centres and widths, exactly
    assert shift == spec.DESIGN_SHIFT
    assert taps.dtype == np.int16 and np.array_equal(taps, want_taps)
    spec.check(taps, shift)                          # what comes out is what sgx_if_filter takes
    if not want_lines:
        ident = np.zeros(L, dtype=np.int16)
        ident[(L - 1) // 2] = 1 << shift
        assert np.array_equal(taps, ident)


def test_nine_lines_drop_the_weakest(built):
    f, pxx = spectrum(NINE)
    _, _, lines = built._native.notch_design(built.Settings(), f, pxx, 8.0, 80e3, 1025)
    centres = [round(c / 1e6 / (f[1] - f[0])) for c, _ in lines]
    assert centres == [b for b, _, _ in NINE[1:]]    # ascending frequency, NINE[0] (14 dB, the weakest) is gone


def test_wide_line_gets_a_wider_notch(built):
    f, pxx = spectrum(CASES["two lines, one of them wide"][0])
    _, _, lines = built._native.notch_design(built.Settings(), f, pxx, 8.0, 80e3, 1025)
    df = (f[1] - f[0]) * 1e6
    assert lines[0][1] == 80e3 and 80e3 < lines[1][1] <= 62 * df


def _design_rc(n, st, f, pxx, n_bins, thr, width, L, null=None):
    taps = np.zeros(4096, dtype=np.int16)
    hz, wd = np.zeros(8), np.zeros(8)
    shift, nl = C.c_int32(0), C.c_int32(0)
    args = [C.byref(st), n._ptr(f), n._ptr(pxx), n_bins, thr, width, L, n._ptr(taps), C.byref(shift), n._ptr(hz),
            n._ptr(wd), C.byref(nl)]
    if null is not None:
        args[null] = None
    return n.lib().sgx_notch_design(*args)


def test_design_refusals(built):
    n = built._native
    st = n.settings_struct(built.Settings())
    f, pxx = spectrum([(2100, 30.0, 1)])
    assert _design_rc(n, st, f, pxx, N_BINS, 8.0, 80e3, 1025) == n.SGX_OK
    for L in (0, -1, 2, 1024, 4096, 4097):
        assert _design_rc(n, st, f, pxx, N_BINS, 8.0, 80e3, L) == n.SGX_E_ARG, L
    assert _design_rc(n, st, f, pxx, 1, 8.0, 80e3, 1025) == n.SGX_E_ARG
    assert _design_rc(n, st, f, pxx, N_BINS, float("nan"), 80e3, 1025) == n.SGX_E_ARG
    for width in (0.0, -1.0, float("inf"), float("nan")):
        assert _design_rc(n, st, f, pxx, N_BINS, 8.0, width, 1025) == n.SGX_E_ARG, width
    for null in (0, 1, 2, 7, 8, 9, 10, 11):
        assert _design_rc(n, st, f, pxx, N_BINS, 8.0, 80e3, 1025, null=null) == n.SGX_E_ARG, null
    bad = pxx.copy()
    bad[17] = np.nan
    assert _design_rc(n, st, f, bad, N_BINS, 8.0, 80e3, 1025) == n.SGX_E_ARG
    # a notch as wide as the band: the centre tap would leave what the filter takes ... or not; either way never garbage
    rc = _design_rc(n, st, f, pxx, N_BINS, 8.0, 30e6, 1025)
    assert rc in (n.SGX_OK, n.SGX_E_ARG)


def _filter_rc(n, taps, shift, n_taps=None):
    h = np.ascontiguousarray(taps, dtype=np.int16)
    out = C.c_void_p()
    return n.lib().sgx_if_filter(None, None, n._ptr(h), h.size if n_taps is None else n_taps, shift, C.byref(out))


def test_filter_refuses_bad_taps_before_it_looks_at_the_device(built):
    """The tap preconditions of the contract are checked first, so they can be shown without a GPU: each refusal is
    SGX_E_ARG and names its own condition; good taps get as far as the missing context."""
    n = built._native
    ident = np.zeros(1025, dtype=np.int16)
    ident[512] = 1 << 14
    assert _filter_rc(n, ident, 14) == n.SGX_E_ARG and "c && in && out" in n.last_error()
    for L in (0, 2, 1024, 4096, 4097):
        assert _filter_rc(n, np.zeros(4097, dtype=np.int16), 14, n_taps=L) == n.SGX_E_ARG
        assert "n_taps" in n.last_error(), L
    for shift in (-1, 31):
        assert _filter_rc(n, ident, shift) == n.SGX_E_ARG and "shift" in n.last_error()
    for v in (32513, -32513, 32767, -32768):
        big = ident.copy()
        big[3] = v
        assert _filter_rc(n, big, 14) == n.SGX_E_ARG and "32512" in n.last_error(), v
    for v in (32512, -32512):
        big = ident.copy()
        big[3] = v
        assert _filter_rc(n, big, 14) == n.SGX_E_ARG and "c && in && out" in n.last_error(), v
    # 128 sum|h| < 2^31: sum|h| = 2^24 - 1 passes, 2^24 does not
    full = np.full(4095, 4097, dtype=np.int16)          # 4095 * 4097 = 2^24 - 1
    assert 128 * int(np.abs(full.astype(np.int64)).sum()) == 2 ** 31 - 128
    assert _filter_rc(n, full, 0) == n.SGX_E_ARG and "c && in && out" in n.last_error()
    full[0] += 1
    assert _filter_rc(n, full, 0) == n.SGX_E_ARG and "2^31" in n.last_error()
    with pytest.raises(ValueError):
        spec.check(full, 0)
    assert n.lib().sgx_filter_timing(None, None) == n.SGX_E_ARG


def test_contract_apply_properties():
    """The contract itself: identity, zero-phase alignment, the rails, and the byte split of a tap."""
    rng = np.random.default_rng(7)
    x = rng.integers(-128, 128, 1000).astype(np.int8)
    ident = np.zeros(33, dtype=np.int16)
    ident[16] = 1 << 5
    assert np.array_equal(spec.apply(x, ident, 5), np.clip(x, -127, 127))
    delay = np.zeros(33, dtype=np.int16)
    delay[16 + 3] = 1
    y = spec.apply(x, delay, 0)                       # h[c + 3] picks x[n - 3]
    assert np.array_equal(y[3:], np.clip(x[:-3], -127, 127)) and not y[:3].any()
    h = rng.integers(-32512, 32513, 4001)
    hi, lo = spec.split(h)
    assert np.array_equal(256 * hi.astype(np.int64) + lo, h)
    assert np.array_equal(spec.apply(x, np.array([300], dtype=np.int16), 0), np.where(x > 0, 127, np.where(x < 0, -127, 0)))
