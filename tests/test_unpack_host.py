"""CPU-only checks of the unpacker (include/sgx.h: sgx_unpack_table, and the argument refusals of sgx_if_unpack that need no
device) against the numpy contract of tests/unpack_spec.py; the contract's own pack / unpack round trips; the exports; the
Settings surface and the skip arithmetic; and the packed records of tests/unpack_cases.py shown to be
well conditioned by the contracts plus the oracle alone.

One refusal of the C ABI looks at the record itself - fields that do not fill whole frames - and a record exists only on a
device: here the contract's own check raises on it, the library's refusal and its text are in tests/test_unpack_gpu.py."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import iq_cases
import unpack_cases as cases
import unpack_spec as spec
from conftest import ROOT, pkg

NEW_SYMBOLS = ("sgx_if_unpack", "sgx_unpack_table", "sgx_unpack_tile", "sgx_unpack_timing")


@pytest.fixture(scope="module")
def built():
    importlib.import_module("__graft_entry__").build()
    return pkg()


def selections(frame):
    return [(first, take) for first in range(frame) for take in range(1, frame - first + 1)]


def test_pack_and_unpack_round_trips():
    """Every (bits, order, frame, first, take): the codes that went into pack() come out of the selection, in order, through
    the table; the counts are the selection's histogram."""
    rng = np.random.default_rng(11)
    for bits in spec.BITS:
        for flags in (0, spec.LSB_FIRST):
            c = rng.integers(0, 1 << bits, 16 * 24)
            b = spec.pack(c, bits, flags)
            assert b.dtype == np.uint8 and b.size == c.size * bits // 8
            assert np.array_equal(spec.codes(b, bits, flags), c)
            table = rng.permutation(256)[:1 << bits] - 128
            for frame in spec.FRAMES:
                for first, take in selections(frame):
                    want = c.reshape(-1, frame)[:, first:first + take].reshape(-1)
                    got = spec.unpack(b, bits, table, flags, frame, first, take)
                    assert got.dtype == np.int8 and np.array_equal(got, table[want]), (bits, flags, frame, first, take)
                    counts = spec.code_counts(b, bits, flags, frame, first, take)
                    assert counts.shape == (16,) and np.array_equal(counts, np.bincount(want, minlength=16))
                    assert counts.sum() == want.size and not counts[1 << bits:].any()
    # by hand: 0xB4 = 10 11 01 00; first field in the high bits, or in the low bits
    assert list(spec.codes(np.array([0xB4], dtype=np.uint8), 2)) == [2, 3, 1, 0]
    assert list(spec.codes(np.array([0xB4], dtype=np.uint8), 2, spec.LSB_FIRST)) == [0, 1, 3, 2]
    assert list(spec.codes(np.array([0xB4], dtype=np.uint8), 4)) == [11, 4]
    assert list(spec.codes(np.array([0xB4], dtype=np.uint8), 1)) == [1, 0, 1, 1, 0, 1, 0, 0]
    for bad in (dict(bits=3), dict(bits=2, flags=2), dict(bits=2, frame=3), dict(bits=2, frame=4, first=3, take=2),
                dict(bits=2, frame=4, take=0), dict(bits=2, frame=4, first=-1), dict(bits=1, frame=16, n_bytes=3),
                dict(bits=4, frame=4, n_bytes=5)):
        with pytest.raises(ValueError):
            spec.check(**bad)
    spec.check(bits=2, frame=2, n_bytes=3)                                     # frames inside a byte: any length


def test_exports(built):
    n = built._native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sgx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(n.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in n.SYMBOLS and hasattr(lib, s), s
    assert (n.UNPACK_LSB_FIRST, n.UNPACK_ENCODINGS) == (spec.LSB_FIRST, spec.ENCODINGS)
    for name, value in (("SGX_UNPACK_LSB_FIRST", 1), ("SGX_UNPACK_SIGN_MAGNITUDE", 0), ("SGX_UNPACK_OFFSET_BINARY", 1),
                        ("SGX_UNPACK_TWOS_COMPLEMENT", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert n.unpack_tile() > 0 and n.unpack_tile() % 16 == 0
    assert "tests/unpack_spec.py" in open(os.path.join(ROOT, "include", "sgx.h")).read()


def test_table_equals_the_contract(built):
    n = built._native
    f = n.lib().sgx_unpack_table
    for bits in spec.BITS:
        for name, enc in spec.ENCODINGS.items():
            lv = spec.levels(bits, enc)
            assert sorted(lv) == list(range(-(1 << bits) + 1, 1 << bits, 2))   # every odd level once
            for peak in range(1, 128):
                buf = np.full(16, 99, dtype=np.int8)
                rc = f(bits, enc, peak, buf.ctypes.data_as(C.c_void_p))
                if peak < (1 << bits) - 1:
                    assert rc == n.SGX_E_ARG and "peak" in n.last_error(), (bits, name, peak)
                    with pytest.raises(ValueError):
                        spec.table(bits, enc, peak)
                    continue
                want = spec.table(bits, enc, peak)
                assert rc == n.SGX_OK and np.array_equal(buf[:1 << bits], want) and np.all(buf[1 << bits:] == 99)
                assert np.array_equal(n.unpack_table(bits, name, peak), want)
                assert np.abs(want.astype(int)).max() == (peak // ((1 << bits) - 1)) * ((1 << bits) - 1) <= peak
    assert list(n.unpack_table(2, "sign-magnitude", 48)) == [16, 48, -16, -48]
    assert list(n.unpack_table(2)) == [16, 48, -16, -48]                       # the defaults
    assert list(n.unpack_table(1, "offset-binary", 48)) == [-48, 48]
    assert list(n.unpack_table(1, "sign-magnitude", 48)) == [48, -48]
    assert list(n.unpack_table(2, "twos-complement", 3)) == [1, 3, -3, -1]
    assert list(n.unpack_table(4, "offset-binary", 127)) == [8 * v for v in range(-15, 16, 2)]
    buf = np.zeros(16, dtype=np.int8)
    p = buf.ctypes.data_as(C.c_void_p)
    for bits in (0, 3, 8, -1):
        assert f(bits, 0, 48, p) == n.SGX_E_ARG and "bits" in n.last_error(), bits
        with pytest.raises(ValueError):
            spec.table(bits, 0, 48)
    for enc in (-1, 3, 100):
        assert f(2, enc, 48, p) == n.SGX_E_ARG and "encoding" in n.last_error(), enc
        with pytest.raises(ValueError):
            spec.table(2, enc, 48)
    for peak in (0, 2, 128, -5):
        assert f(2, 0, peak, p) == n.SGX_E_ARG and "peak" in n.last_error(), peak
    assert f(2, 0, 48, None) == n.SGX_E_ARG and "table" in n.last_error()
    with pytest.raises(ValueError, match="encoding"):
        n.unpack_table(2, "gray", 48)


def _unpack_rc(n, bits=2, flags=0, frame=1, first=0, take=1, table=True, out=True):
    tab = np.zeros(16, dtype=np.int8)
    h = C.c_void_p()
    return n.lib().sgx_if_unpack(None, None, bits, flags, frame, first, take,
                                 tab.ctypes.data_as(C.c_void_p) if table else None, C.byref(h) if out else None, None)


def test_refusals_before_the_device(built):
    """Every precondition that needs no record: each refusal is SGX_E_ARG and names its argument (and the contract's check
    raises on it); good arguments get as far as the missing context."""
    n = built._native
    assert _unpack_rc(n) == n.SGX_E_ARG and "c && rec && table && out" in n.last_error()
    for bits in (0, 3, 5, 8, -1):
        assert _unpack_rc(n, bits=bits) == n.SGX_E_ARG and "bits" in n.last_error(), bits
    for flags in (2, 3, 4, -1, 1 << 16):
        assert _unpack_rc(n, flags=flags) == n.SGX_E_ARG and "flags" in n.last_error(), flags
        with pytest.raises(ValueError):
            spec.check(2, flags)
    assert _unpack_rc(n, flags=1) == n.SGX_E_ARG and "c && rec" in n.last_error()
    for frame in (0, 3, 5, 6, 12, 32, -4):
        assert _unpack_rc(n, frame=frame) == n.SGX_E_ARG and "frame" in n.last_error(), frame
    for frame in spec.FRAMES:
        for first, take in selections(frame):
            assert _unpack_rc(n, frame=frame, first=first, take=take) == n.SGX_E_ARG and "c && rec" in n.last_error()
        for first, take in ((0, 0), (0, -1), (-1, 1), (0, frame + 1), (frame, 1), (frame - 1, 2), (1, 2 ** 31 - 1)):
            assert _unpack_rc(n, frame=frame, first=first, take=take) == n.SGX_E_ARG
            assert "first" in n.last_error() and "take" in n.last_error(), (frame, first, take)
            with pytest.raises(ValueError):
                spec.check(2, 0, frame, first, take)
    assert _unpack_rc(n, table=False) == n.SGX_E_ARG and "table" in n.last_error()
    assert _unpack_rc(n, out=False) == n.SGX_E_ARG and "out" in n.last_error()
    assert n.lib().sgx_unpack_timing(None, None) == n.SGX_E_ARG and "kernel_ms" in n.last_error()
    assert n.lib().sgx_unpack_tile(None) == n.SGX_E_ARG and "tile_bytes" in n.last_error()


def test_settings_surface(built):
    s = built.Settings()
    assert (s.packedBits, s.packedEncoding, s.packedLsbFirst, s.packedFrame, s.packedFirst, s.packedPeak, s.packedTable) == \
        (0, 'sign-magnitude', False, 1, 0, 48, None)
    assert s.packedPeak == spec.DEFAULT_PEAK
    assert s._prepared_settings() is s                                         # off: nothing on any existing path changes
    with pytest.raises(ValueError, match="packedBits"):
        s.unpackRecord(None)
    with pytest.raises(ValueError, match="packedBits"):
        s._pack_format()
    # what the unpacker is called with
    s.packedBits = 2
    b, lsb, F, first, take, table = s._pack_format()
    assert (b, lsb, F, first, take) == (2, False, 1, 0, 1) and list(table) == [16, 48, -16, -48]
    s.iqRecord, s.samplingFreq, s.IF = True, 4096000.0, 0.0
    assert s._pack_format()[4] == 1                                            # I and Q simply alternate
    s.packedFrame, s.packedFirst = 4, 2
    assert s._pack_format()[2:5] == (4, 2, 2)                                  # the second antenna's pair
    s.iqRecord = False
    assert s._pack_format()[2:5] == (4, 2, 1)                                  # one stream of four
    s.packedFrame, s.packedFirst = 1, 0
    s.packedEncoding, s.packedPeak, s.packedLsbFirst = 'twos-complement', 63, True
    assert list(s._pack_format()[5]) == list(spec.table(2, spec.TWOS_COMPLEMENT, 63)) and s._pack_format()[1] is True
    s.packedTable = [5, -7, 127, -128]                                         # overrides encoding and peak
    s.packedEncoding, s.packedPeak = 'gray', 1000
    assert list(s._pack_format()[5]) == [5, -7, 127, -128] and s._pack_format()[5].dtype == np.int8
    for bad in ([1, 2, 3], [1, 2, 3, 128], [1.5, 2, 3, 4], [[1, 2], [3, 4]]):
        s.packedTable = bad
        with pytest.raises(ValueError, match="packedTable"):
            s._pack_format()
    s.packedTable = None
    with pytest.raises(ValueError, match="packedEncoding"):
        s._pack_format()
    s.packedEncoding = 'offset-binary'
    with pytest.raises(ValueError, match="packedPeak"):
        s._pack_format()
    for bits, peak in ((1, 0), (2, 2), (4, 14), (4, 128)):
        s.packedBits, s.packedPeak = bits, peak
        with pytest.raises(ValueError, match="packedPeak"):
            s._pack_format()
    s.packedPeak = 48
    # the combinations that are refused, with the reason
    for bits in (3, 8, -1):
        s.packedBits = bits
        with pytest.raises(ValueError, match="packedBits"):
            s.postProcessing("/nonexistent/record.bin")
    s.packedBits = 2
    s.iqRecord, s.iqRequantize = True, True
    with pytest.raises(ValueError, match="iqRequantize"):
        s.postProcessing("/nonexistent/record.bin")
    s.iqRequantize, s.frontEndConditioning = False, True
    with pytest.raises(ValueError, match="frontEndConditioning"):
        s.postProcessing("/nonexistent/record.bin")
    s.frontEndConditioning = False
    for dt in ('uint8', 'int16', 'float32'):
        s.dataType = dt
        with pytest.raises(ValueError, match="dataType"):
            s.postProcessing("/nonexistent/record.bin")
    s.dataType = 'int8'
    for frame in (0, 3, 32):
        s.packedFrame = frame
        with pytest.raises(ValueError, match="packedFrame"):
            s._prepared_settings()
    s.packedFrame = 4
    for first in (-1, 3, 4):                                                   # with iqRecord two fields are taken
        s.packedFirst = first
        with pytest.raises(ValueError, match="packedFirst"):
            s._prepared_settings()
    s.iqRecord, s.packedFirst = False, 3
    assert s._pack_format()[2:5] == (4, 3, 1)
    # iqRecord and interferenceMitigation compose with it
    s.iqRecord, s.packedFirst, s.interferenceMitigation = True, 2, True
    real = s._prepared_settings()
    assert (real.packedBits, real.iqRecord, real.dataType, real.samplingFreq, real.IF) == (0, False, 'int8', 8192000.0,
                                                                                            2048000.0)
    assert s.packedBits == 2 and s.iqRecord                                    # left alone


def test_skip_arithmetic(built):
    """skipNumberOfBytes is a byte of the packed file on a frame boundary, a multiple of max(1, F b / 8); it becomes sample
    skip 8 take / (b F) of the prepared record."""
    for bits in spec.BITS:
        for frame in spec.FRAMES:
            for iq in (False, True):
                s = built.Settings()
                s.packedBits, s.packedFrame, s.iqRecord, s.samplingFreq, s.IF = bits, frame, iq, 4096000.0, 0.0
                take = 2 if iq and frame > 1 else 1
                unit = max(1, frame * bits // 8)
                assert s._pack_units() == (unit, unit * 8 * take // (bits * frame))
                assert not iq or s._pack_units()[1] % 2 == 0                   # whole frames hold whole I/Q pairs
                for k in (0, 1, 5, 1000):
                    s.skipNumberOfBytes = k * unit
                    real = s._prepared_settings()
                    assert real.skipNumberOfBytes * bits * frame == k * unit * 8 * take, (bits, frame, iq, k)
                    assert not iq or real.skipNumberOfBytes % 2 == 0           # whole I/Q pairs
                    assert real.packedBits == 0 and real.dataType == 'int8' and not real.iqRecord
                    assert s.skipNumberOfBytes == k * unit
                for skip in (1, unit - 1, unit + 1, 3 * unit + unit // 2):
                    if skip % unit:
                        s.skipNumberOfBytes = skip
                        with pytest.raises(ValueError, match="skipNumberOfBytes = %d" % skip):
                            s._prepared_settings()
                        with pytest.raises(ValueError, match="skipNumberOfBytes = %d" % skip):
                            s.postProcessing("/nonexistent/record.bin")
    for case in cases.CASES.values():
        assert case.file_bytes(cases.SKIP_SAMPLES) % max(1, case.frame * case.bits // 8) == 0
        s = case.settings(built, skipNumberOfBytes=case.file_bytes(cases.SKIP_SAMPLES))
        assert s._prepared_settings().skipNumberOfBytes == cases.SKIP_SAMPLES


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_packed_records_are_well_conditioned(name):
    """The contracts' record under the oracle's search: exactly the scene's satellites, where the scene put them, with
    iq_cases.MARGIN to spare - the precondition of the end-to-end tests on the GPU."""
    case, scene = cases.CASES[name], cases.SCENE
    b = cases.file_of(case, 11)
    assert b.size == case.file_bytes(11 * scene.samples_per_code)
    y8 = cases.unpacked(case, b)
    assert y8.size == 11 * scene.samples_per_code and set(np.unique(y8)) <= set(case.table.tolist())
    shares = spec.code_counts(b, case.bits, case.flags, case.frame, case.first, case.take)[:1 << case.bits] / float(y8.size)
    print("%s: level shares %s" % (name, ", ".join("%+d: %.3f" % (lv, sh) for lv, sh in sorted(zip(case.table, shares)))))
    if case.bits == 2:                                                         # about a third in the outer levels
        outer = shares[np.abs(case.table.astype(int)) == 48].sum()
        assert 0.28 < outer < 0.38, outer
    y = cases.contract_record(case, 11)
    a = np.abs(y.astype(np.int64))
    win = np.concatenate(([0], np.cumsum(a)))
    print("%s: max |y| %d, largest 2048-sample sum of magnitudes %d" % (name, a.max(), (win[2048:] - win[:-2048]).max()))
    assert (win[2048:] - win[:-2048]).max() < 131072                           # tracking stays on its fastest kernel
    ref = cases.contract_acquisition(case)
    o = scene.oracle_settings()
    assert sorted(np.flatnonzero(ref["carrFreq"]) + 1) == sorted(scene.prns)
    others = np.delete(ref["peakMetric"], [p - 1 for p in scene.prns])
    print("%s: largest peak metric among the other 28 PRNs %.2f" % (name, float(others.max())))
    for i, prn in enumerate(scene.prns):
        f, c, pm = ref["carrFreq"][prn - 1], ref["codePhase"][prn - 1], ref["peakMetric"][prn - 1]
        print("%s PRN %2d: carrFreq %+.1f Hz, code phase %+.2f samples off the truth, peak metric %.1f"
              % (name, prn, f - scene.true_carrier(i), c - scene.code_start[i], pm))
        assert abs(f - scene.true_carrier(i)) <= iq_cases.CARR_TOL_HZ
        assert abs(c - scene.code_start[i]) <= iq_cases.PHASE_TOL
        assert pm >= iq_cases.MARGIN * o.acqThreshold
