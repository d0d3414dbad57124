"""CPU-only checks of the requantiser in front of the I/Q converter (include/sgx.h: sgx_requant_gain, and the argument
refusals of sgx_requant_stats_of / sgx_if_requantize that need no device) against the numpy contract of
tests/requant_spec.py; the exports and the struct layout; the Settings surface; and the int16 and
float32 captures of tests/requant_cases.py shown to be well conditioned by the contracts plus the oracle alone.

Two refusals of the C ABI look at the record itself - N not a multiple of the element width, a window that leaves the
record - and a record exists only on a device: here the contract's own checks raise on them, the library's refusals and
their texts are in tests/test_requant_gpu.py."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import iq_cases
import requant_cases as cases
import requant_spec as spec
from conftest import ROOT, pkg

NEW_SYMBOLS = ("sgx_if_requantize", "sgx_requant_gain", "sgx_requant_stats_of", "sgx_requant_tile", "sgx_requant_timing")


@pytest.fixture(scope="module")
def built():
    importlib.import_module("__graft_entry__").build()
    return pkg()


def test_exports_and_layout(built):
    n = built._native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sgx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(n.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in n.SYMBOLS and hasattr(lib, s), s
    # typedef struct { int64_t n_finite, n_nonfinite; double max_abs, sum, sum_sq; } sgx_requant_stats
    m = re.search(r"typedef struct sgx_requant_stats \{(.*?)\} sgx_requant_stats;", text, flags=re.S)
    fields = [f.strip() for decl in m.group(1).split(";") if decl.strip()
              for f in decl.replace("int64_t", "").replace("double", "").split(",")]
    assert fields == [f[0] for f in n.RequantStats._fields_] == ["n_finite", "n_nonfinite", "max_abs", "sum", "sum_sq"]
    assert C.sizeof(n.RequantStats) == 40
    assert [getattr(n.RequantStats, f).offset for f in fields] == [0, 8, 16, 24, 32]
    assert (n.DT_INT16, n.DT_FLOAT32) == (1, 3) and n.requant_type("int16") == (1, 2) and n.requant_type("<f4") == (3, 4)
    assert n.requant_tile() > 0 and n.requant_tile() % 16 == 0
    assert "tests/requant_spec.py" in open(os.path.join(ROOT, "include", "sgx.h")).read()


def _ulp_neighbours(x, k=2):
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo, hi = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
        out += [lo, hi]
    return out


def gain_table():
    """(n_finite, sum_sq, target_rms): rms over 60 decades; gains whose g 2^S lies next to 32767.5 (where S steps down) and
    next to half-even ties k + 1/2 for k of both parities; rms = 0, no finite sample, a tiny and a huge rms."""
    rows = [(0, 0.0, 12.0), (0, 25.0, 12.0), (1000, 0.0, 12.0), (1, 1e-300, 12.0), (1000, 1e-40, 12.0), (1, 1e300, 12.0),
            (1000, 1e40, 12.0), (5, 4.0 * 5, 127.0), (7, 1.0 * 7, 1e-6)]
    rng = np.random.default_rng(5)
    for rms in np.exp(rng.uniform(-70.0, 70.0, 400)):
        rows.append((1000, float(rms) ** 2 * 1000, float(rng.choice([12.0, 1.0, 127.0, 33.3]))))
    # n_finite = 1, sum_sq = rms^2 with rms a power of two: sqrt and the division are exact, g = target / rms exactly
    for S in (0, 1, 7, 14, 29, 30):
        for frac in (32767.5, 32766.5, 16384.5, 16385.5, 20000.5, 20001.5, 32767.0, 32768.0):
            for t in _ulp_neighbours(frac * 2.0 ** -20):      # target in (0, 127]; g 2^S = t 2^20 -> rms = 2^(S - 20)
                rows.append((1, (2.0 ** (S - 20)) ** 2, t))
    return rows


def test_gain_equals_the_contract(built):
    n = built._native
    seen_ties = seen_max = 0
    for n_finite, sum_sq, target in gain_table():
        want = spec.gain(n_finite, sum_sq, target)
        for dt in ("int16", "float32"):
            got = n.requant_gain(dict(n_finite=n_finite, sum_sq=sum_sq), dt, target)
            assert (got[0], got[1]) == (want[0], want[1]), (n_finite, sum_sq, target, got, want)
            assert np.float32(got[2]).tobytes() == np.float32(want[2]).tobytes(), (n_finite, sum_sq, target, got, want)
        assert 1 <= want[0] <= 32767 and 0 <= want[1] <= 30 and spec.SCALE_MIN <= float(want[2]) <= spec.SCALE_MAX
        spec.check_gain("int16", want[0], want[1])
        spec.check_gain("float32", scale=float(want[2]))
        seen_max += want[0] == 32767
        g = target / math.sqrt(sum_sq / n_finite) if n_finite and sum_sq > 0 else 1.0
        seen_ties += math.ldexp(g, want[1]) % 1.0 == 0.5
    assert seen_max >= 4 and seen_ties >= 8          # the table does sit on the boundaries it claims
    # by hand: g = 1; g = 12 / 500; the tie 20000.5 rounds to even, 20001.5 to 20002; 32767.5 -> 32768 steps S down
    assert spec.gain(0, 0.0) == (16384, 14, np.float32(1.0)) and spec.gain(10, 0.0)[:2] == (16384, 14)
    assert spec.gain(1, 500.0 ** 2, 12.0)[:2] == (int(np.rint(0.024 * 2 ** 20)), 20)
    assert spec.gain(1, 1.0, 20000.5 * 2.0 ** -10)[:2] == (20000, 10)
    assert spec.gain(1, 1.0, 20001.5 * 2.0 ** -10)[:2] == (20002, 10)
    assert spec.gain(1, 1.0, 32767.5 * 2.0 ** -10)[:2] == (16384, 9)
    assert spec.gain(1, 1e-40, 12.0)[:2] == (32767, 0) and spec.gain(1, 1e-300, 12.0)[2] == np.float32(2.0 ** 100)
    assert spec.gain(1, 1e300, 12.0)[:2] == (1, 30) and spec.gain(1, 1e300, 12.0)[2] == np.float32(2.0 ** -100)
    # the product the quantiser forms stays inside int32 for every gain there is
    assert 32768 * 32767 + (1 << 29) < 2 ** 31


def _requantize_rc(n, data_type, mult=1, shift=0, scale=1.0):
    out = C.c_void_p()
    return n.lib().sgx_if_requantize(None, None, data_type, mult, shift, scale, C.byref(out), None)


def test_refusals_before_the_device(built):
    """Every precondition that needs no record: each refusal is SGX_E_ARG and names its argument (and the contract's
    checks raise on it); good arguments get as far as the missing context."""
    n = built._native
    f = n.lib()
    st = n.RequantStats(100, 0, 50.0, 0.0, 100.0 * 40.0 ** 2)
    m, sh, sc = C.c_int32(0), C.c_int32(0), C.c_float(0)
    assert f.sgx_requant_gain(C.byref(st), n.DT_INT16, 12.0, C.byref(m), C.byref(sh), C.byref(sc)) == n.SGX_OK
    # data_type
    for dt in (n.DT_INT8, n.DT_UINT8, n.DT_FLOAT64, n.DT_UINT16, n.DT_FLOAT16, -1, 11):
        assert f.sgx_requant_gain(C.byref(st), dt, 12.0, C.byref(m), C.byref(sh), C.byref(sc)) == n.SGX_E_ARG
        assert "data_type" in n.last_error(), dt
        assert _requantize_rc(n, dt) == n.SGX_E_ARG and "data_type" in n.last_error(), dt
        assert f.sgx_requant_stats_of(None, None, dt, 0, 0, C.byref(st)) == n.SGX_E_ARG and "data_type" in n.last_error()
    for name in ("int8", "uint8", "uint16", "float64", "complex64"):
        with pytest.raises(ValueError):
            spec.width(name)
        with pytest.raises(ValueError):
            n.requant_type(name)
    # target_rms
    for t in (0.0, -1.0, 127.0000001, 1e9, float("nan"), float("inf")):
        assert f.sgx_requant_gain(C.byref(st), n.DT_INT16, t, C.byref(m), C.byref(sh), C.byref(sc)) == n.SGX_E_ARG
        assert "target_rms" in n.last_error(), t
        with pytest.raises(ValueError):
            spec.gain(100, 1.0, t)
    assert f.sgx_requant_gain(C.byref(st), n.DT_FLOAT32, 127.0, C.byref(m), C.byref(sh), C.byref(sc)) == n.SGX_OK
    # NULL pointers
    args = [C.byref(st), n.DT_INT16, 12.0, C.byref(m), C.byref(sh), C.byref(sc)]
    for i, name in ((0, "st"), (3, "mult"), (4, "shift"), (5, "scale")):
        a = list(args)
        a[i] = None
        assert f.sgx_requant_gain(*a) == n.SGX_E_ARG and name in n.last_error(), name
    assert f.sgx_requant_stats_of(None, None, n.DT_INT16, 0, 0, C.byref(st)) == n.SGX_E_ARG
    assert "c && rec && out" in n.last_error()
    assert f.sgx_requant_timing(None, None, None) == n.SGX_E_ARG and "stats_ms" in n.last_error()
    assert f.sgx_requant_tile(None) == n.SGX_E_ARG and "tile_bytes" in n.last_error()
    # mult and shift (int16), scale (float32): good ones get as far as the missing context
    assert _requantize_rc(n, n.DT_INT16, 1, 0) == n.SGX_E_ARG and "c && rec && out" in n.last_error()
    assert _requantize_rc(n, n.DT_INT16, 32767, 30) == n.SGX_E_ARG and "c && rec && out" in n.last_error()
    for mult in (0, -1, 32768, 1 << 20):
        assert _requantize_rc(n, n.DT_INT16, mult, 3) == n.SGX_E_ARG and "mult" in n.last_error(), mult
        with pytest.raises(ValueError):
            spec.check_gain("int16", mult, 3)
    for shift in (-1, 31, 64):
        assert _requantize_rc(n, n.DT_INT16, 5, shift) == n.SGX_E_ARG and "shift" in n.last_error(), shift
        with pytest.raises(ValueError):
            spec.check_gain("int16", 5, shift)
    for scale in (2.0 ** -100, 2.0 ** 100, 1.0, 0.0234375):
        assert _requantize_rc(n, n.DT_FLOAT32, scale=scale) == n.SGX_E_ARG and "c && rec && out" in n.last_error(), scale
    for scale in (0.0, -1.0, 2.0 ** -101, 2.0 ** 101, float("nan"), float("inf"), -float("inf")):
        assert _requantize_rc(n, n.DT_FLOAT32, scale=scale) == n.SGX_E_ARG and "scale" in n.last_error(), scale
        with pytest.raises(ValueError):
            spec.check_gain("float32", scale=scale)
    # the two refusals that look at the record: the contract's side (the library's: tests/test_requant_gpu.py)
    for dt, nbytes in (("int16", 7), ("float32", 6), ("float32", 9)):
        with pytest.raises(ValueError):
            spec.elements(np.zeros(nbytes, dtype=np.uint8), dt)
    for off, cnt in ((11, 0), (0, 11), (5, 6), (10, 1)):
        with pytest.raises(ValueError):
            spec.stats(np.zeros(10, dtype="<i2"), "int16", off, cnt)
    assert spec.stats(np.zeros(10, dtype="<i2"), "int16", 10, 0)["n_finite"] == 0


def test_contract_closed_forms():
    """The quantiser and the statistics where they can be written down by hand."""
    x = np.array([-32768, -32767, -255, -129, -128, -127, -3, -2, -1, 0, 1, 2, 3, 126, 127, 128, 32767], dtype="<i2")
    assert list(spec.quantise(x, "int16", 1, 0)) == [-127, -127, -127, -127, -127, -127, -3, -2, -1, 0, 1, 2, 3, 126, 127, 127,
                                                     127]
    assert np.array_equal(spec.quantise(x, "int16", 16384, 14), spec.quantise(x, "int16", 1, 0))
    # (1, 1): (x + 1) >> 1 - ties go up; (3, 2): (3 x + 2) >> 2, a tie at every x = 2 mod 4
    assert list(spec.quantise(np.array([-3, -2, -1, 0, 1, 2, 3], dtype="<i2"), "int16", 1, 1)) == [-1, -1, 0, 0, 1, 1, 2]
    assert list(spec.quantise(np.array([-6, -2, 2, 6], dtype="<i2"), "int16", 3, 2)) == [-4, -1, 2, 5]
    assert list(spec.quantise(np.array([-32768, 32767], dtype="<i2"), "int16", 32767, 30)) == [-1, 1]
    f = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.5, 1e30, -1e30, np.inf, -np.inf, np.nan, 1e-45, -0.0],
                 dtype="<f4")
    assert list(spec.quantise(f, "float32", scale=1.0)) == [0, 2, 2, 0, -2, -2, 126, 127, 127, -127, 127, -127, 0, 0, 0]
    st = spec.stats(f, "float32")
    assert (st["n_finite"], st["n_nonfinite"], st["max_abs"]) == (12, 3, float(np.float32(1e30)))
    st = spec.stats(np.array([-32768, 3, -4], dtype="<i2"), "int16", 0, 3)
    assert (st["n_finite"], st["n_nonfinite"], st["max_abs"], st["sum"], st["sum_sq"]) == (3, 0, 32768.0, -32769.0,
                                                                                           2.0 ** 30 + 25.0)
    assert spec.clipped_share(np.array([127, -127, 126, 0], dtype=np.int8)) == 0.5


def test_settings_surface(built):
    s = built.Settings()
    assert (s.iqRequantize, s.iqTargetRms) == (False, 12.0) == (False, spec.DEFAULT_TARGET_RMS)
    s.iqRecord, s.samplingFreq, s.IF = True, 4096000.0, 0.0
    for dt in ('int16', 'float32', 'uint16'):                 # off: as before
        s.dataType = dt
        with pytest.raises(ValueError, match="int8.*not converted"):
            s.postProcessing("/nonexistent/record.bin")
        with pytest.raises(ValueError, match="int8"):
            s._iq_format()
    s.dataType = 'int16'
    with pytest.raises(ValueError, match="iqRequantize"):
        s.requantizeIQ(None)
    s.iqRequantize = True
    for dt, w in (('int16', 2), ('float32', 4), ('<f4', 4), (np.int16, 2)):
        s.dataType = dt
        assert s._iq_format() == (False, False) and s._iq_width() == w
    s.iqQFirst = True
    assert s._iq_format() == (True, False)
    s.iqQFirst = False
    for dt in ('uint16', 'float64', 'int32', 'float16', 'complex64'):
        s.dataType = dt
        with pytest.raises(ValueError, match="int8"):
            s._iq_format()
        with pytest.raises(ValueError, match="int8"):
            s.postProcessing("/nonexistent/record.bin")
    for dt, w in (('int8', 1), ('uint8', 1)):                  # the 8-bit formats stay what they were
        s.dataType = dt
        assert s._iq_width() == w and s._iq_format() == (False, dt == 'uint8')
    # realEquivalent() is unchanged; the prepared record's settings carry the skip as a sample of that record
    s.dataType, s.skipNumberOfBytes = 'float32', 8 * 1000
    real = s.realEquivalent()
    assert (real.samplingFreq, real.IF, real.iqRecord, real.dataType, real.skipNumberOfBytes) == (8192000.0, 2048000.0, False,
                                                                                                 'int8', 8000)
    assert s._prepared_settings().skipNumberOfBytes == 2000 and s.skipNumberOfBytes == 8000
    s.dataType = 'int16'
    assert s._prepared_settings().skipNumberOfBytes == 4000
    for dt, skip in (('int16', 2), ('int16', 6), ('int16', 1), ('float32', 4), ('float32', 12), ('float32', 2)):
        s.dataType, s.skipNumberOfBytes = dt, skip
        with pytest.raises(ValueError, match="skipNumberOfBytes = %d" % skip):
            s.postProcessing("/nonexistent/record.bin")
    s.dataType, s.skipNumberOfBytes = 'int8', 3
    with pytest.raises(ValueError, match="even"):
        s.postProcessing("/nonexistent/record.bin")


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_wide_captures_are_well_conditioned(dtype):
    """The contracts' record under the oracle's search: exactly the scene's satellites, where the scene put them."""
    scene = cases.SCENE
    x = cases.wide_record(dtype, 11)
    st, mult, shift, scale = cases.contract_gain(x)
    rms = math.sqrt(st["sum_sq"] / st["n_finite"])
    print("%s: rms %.6g, peak %.6g, mult %d, shift %d, scale %.6g" % (dtype, rms, st["max_abs"], mult, shift, float(scale)))
    assert (400.0 < rms < 600.0) if dtype == "int16" else (0.9 * 2.0 ** -11 < rms < 1.1 * 2.0 ** -11)
    y8 = spec.quantise(x, x.dtype, mult, shift, scale)
    assert abs(float(np.sqrt(np.mean(y8.astype(np.float64) ** 2))) - cases.TARGET_RMS) < 0.05
    assert spec.clipped_share(y8) == 0.0
    ref = cases.contract_acquisition(dtype)
    o = scene.oracle_settings()
    assert sorted(np.flatnonzero(ref["carrFreq"]) + 1) == sorted(scene.prns)
    for i, prn in enumerate(scene.prns):
        f, c, pm = ref["carrFreq"][prn - 1], ref["codePhase"][prn - 1], ref["peakMetric"][prn - 1]
        print("%s PRN %2d: carrFreq %+.1f Hz, code phase %+.2f samples off the truth, peak metric %.1f"
              % (dtype, prn, f - scene.true_carrier(i), c - scene.code_start[i], pm))
        assert abs(f - scene.true_carrier(i)) <= iq_cases.CARR_TOL_HZ
        assert abs(c - scene.code_start[i]) <= iq_cases.PHASE_TOL
        assert pm >= iq_cases.MARGIN * o.acqThreshold
