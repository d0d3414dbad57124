"""The requantiser on the GPU (sgx_requant_stats_of, sgx_if_requantize, csrc/sgx_requant.hip; Settings.requantizeIQ,
postProcessing with iqRequantize): the quantiser against the numpy contract of tests/requant_spec.py byte for byte, the
statistics exactly (int16, the counts, max_abs) or within the contract's bounds of the correctly rounded sums (float32),
then the int16 and float32 captures of tests/requant_cases.py end to end against the contracts' record and the oracle on
it, by the bars of tests/test_iq_gpu.py.  Run with -m gpu."""
import ctypes as C
import math

import numpy as np
import pytest

import requant_cases as cases
import requant_spec as spec
from conftest import pkg
from oracle import softgnss_oracle as orc
from record_stage import same_tracking

pytestmark = pytest.mark.gpu

TRK_MS = 300
SCENE = cases.SCENE
DTYPES = ("int16", "float32")


@pytest.fixture(scope="module")
def ctx():
    m = pkg()
    return m.engine.get_context(m.Settings(), 0)


@pytest.fixture(scope="module")
def tile():
    return pkg()._native.requant_tile()


def lengths(tile):
    return [0, 1, 2, 3, 15, 16, 17, tile - 1, tile, tile + 1, 3 * tile + 5]


def up(ctx, x):
    """The bytes of x as a resident record (an empty one too)."""
    return ctx.upload(np.frombuffer(np.ascontiguousarray(x).tobytes(), dtype=np.int8))


def same(ctx, x, **gain):
    """x (int16 or float32 elements) through the library equals the contract byte for byte; so does the clip count."""
    want = spec.quantise(x, x.dtype, **gain)
    rec = up(ctx, x)
    try:
        out = ctx.requantize(rec, x.dtype, **gain)
        try:
            assert len(out) == x.size
            got = out.download()
            assert got.tobytes() == want.tobytes(), \
                "%s, n = %d, %r: first difference at element %d" % (x.dtype, x.size, gain, int(np.flatnonzero(got != want)[0]))
            assert out.clipped == np.count_nonzero(np.abs(want.astype(np.int16)) == 127)
        finally:
            out.free()
    finally:
        rec.free()
    return want


# ---- the quantiser ---------------------------------------------------------------------------------------------------------

def int16_pairs():
    n = pkg()._native
    made = [n.requant_gain(dict(n_finite=1000, sum_sq=1000 * rms * rms), "int16", t)[:2] for rms, t in ((504.0, 12.0),
                                                                                                     (9000.0, 40.0))]
    assert made == [spec.gain(1000, 1000 * 504.0 ** 2, 12.0)[:2], spec.gain(1000, 1000 * 9000.0 ** 2, 40.0)[:2]]
    return [(1, 0), (32767, 0), (32767, 30), (16384, 14), (1, 1), (3, 2)] + made


def test_int16_quantiser_is_exhaustive(ctx):
    """All 65 536 values, in order and shuffled, at every (mult, shift) of the list."""
    ordered = np.arange(-32768, 32768).astype("<i2")
    shuffled = np.random.default_rng(2).permutation(ordered)
    for mult, shift in int16_pairs():
        a = same(ctx, ordered, mult=mult, shift=shift)
        b = same(ctx, shuffled, mult=mult, shift=shift)
        assert np.array_equal(np.sort(a), np.sort(b))
    # (16384, 14) is the identity but for the clip; (1, 1) and (3, 2) round ties of either sign up
    y = same(ctx, ordered, mult=16384, shift=14)
    assert np.array_equal(y, np.clip(ordered.astype(np.int64), -127, 127))
    y = same(ctx, np.array([-3, -2, -1, 0, 1, 2, 3, -6, 6], dtype="<i2"), mult=1, shift=1)
    assert list(y) == [-1, -1, 0, 0, 1, 1, 2, -3, 3]
    y = same(ctx, np.array([-6, -2, 2, 6], dtype="<i2"), mult=3, shift=2)
    assert list(y) == [-4, -1, 2, 5]


def float_gains():
    made = pkg()._native.requant_gain(dict(n_finite=1000, sum_sq=1000 * 4.9e-4 ** 2), "float32", 12.0)[2]
    assert np.float32(made).tobytes() == np.float32(spec.gain(1000, 1000 * 4.9e-4 ** 2, 12.0)[2]).tobytes()
    return [2.0 ** -100, 2.0 ** -11, 1.0, 0.0234375, 2.0 ** 100, float(made)]


def hand_vector(gf):
    """The values the contract's corners lie at for this gain, as float32."""
    f32 = np.float32
    v = [0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, np.inf, -np.inf, 3e38, -3e38]
    with np.errstate(all="ignore"):
        for k in (0, 1, 2, 3, 10, 11, 125, 126, 127, 128):                     # (k + 1/2) / gf: ties of both parities
            v += [float(f32((k + 0.5) / gf)), -float(f32((k + 0.5) / gf))]
        for edge in (126.5, 127.5):
            for sgn in (1.0, -1.0):
                c = f32(sgn * edge / gf)
                v += [float(c), float(np.nextafter(c, f32(np.inf))), float(np.nextafter(c, f32(-np.inf)))]
        x = np.array(v, dtype="<f4")
    nan_bits = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0x7FA00000], dtype="<u4")   # quiet, signalling
    return np.concatenate([x, nan_bits.view("<f4")])


def test_float32_quantiser_on_every_kind_of_value(ctx):
    patterns = np.random.default_rng(3).integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype("<u4").view("<f4")
    kinds = patterns.view("<u4")
    assert np.count_nonzero(np.isnan(patterns)) > 1000 and np.count_nonzero((kinds & 0x7F800000) == 0) > 1000   # NaN, denormal
    for gf in float_gains():
        same(ctx, patterns, scale=gf)
        x = hand_vector(gf)
        y = same(ctx, x, scale=gf)
        assert list(y[:10]) == [0, 0, 0, 0, 0, 0, 127, -127, 127, -127] or gf < 2.0 ** -90
        assert not y[-6:].any()                                                # every NaN gives 0
    # gf a power of two: the ties (k + 1/2) / gf are exact and go to the even neighbour
    for gf in (2.0 ** -11, 1.0):
        k = np.array([0, 1, 2, 3, 10, 11, 125, 126], dtype=np.float64)
        x = np.concatenate([(k + 0.5) / gf, -(k + 0.5) / gf]).astype("<f4")
        even = (k + (k % 2)).astype(np.int64)
        assert list(same(ctx, x, scale=gf)) == list(even) + list(-even)
    # values spread over the output range, not only the rails
    x = np.random.default_rng(4).normal(0.0, 40.0, 100000).astype("<f4")
    y = same(ctx, x, scale=1.0)
    assert np.count_nonzero(np.abs(y.astype(int)) < 127) > 90000


# ---- lengths, the record's behaviour -----------------------------------------------------------------------------------------

def sample_record(rng, dtype, n):
    """n elements that spread over the int8 range at the test gains, with a few on either rail."""
    if np.dtype(dtype) == spec.INT16:
        x = np.clip(np.rint(rng.normal(0.0, 500.0, n)), -32768, 32767).astype("<i2")
        x[::97] = -32768
        x[5::101] = 32767
    else:
        x = rng.normal(0.0, 4.9e-4, n).astype("<f4")
        x[::97] = -np.inf
        x[5::101] = np.nan
        x[7::103] = 1e-41
    return x


GAIN = {"int16": dict(mult=24969, shift=20), "float32": dict(scale=24512.5)}


@pytest.mark.parametrize("dtype", DTYPES)
def test_lengths_and_record_behaviour(ctx, tile, tmp_path, dtype):
    n = pkg()._native
    rng = np.random.default_rng(20)
    for ln in lengths(tile):
        x = sample_record(rng, dtype, ln)
        want = same(ctx, x, **GAIN[dtype])
        assert want.size == ln
    x = sample_record(rng, dtype, 3 * tile + 5)
    want = spec.quantise(x, x.dtype, **GAIN[dtype])
    rec = up(ctx, x)
    try:
        a = ctx.requantize(rec, dtype, **GAIN[dtype])
        b = ctx.requantize(rec, dtype, **GAIN[dtype])
        assert rec.download().tobytes() == x.tobytes()                          # the input is left alone
        ln = C.c_size_t(0)
        assert n.lib().sgx_if_length(a._h, C.byref(ln)) == n.SGX_OK and ln.value == x.size == len(a)
        assert a.download().tobytes() == want.tobytes() == b.download().tobytes() and a.clipped == b.clipped
        assert a.download(tile - 3, 11).tobytes() == want[tile - 3:tile + 8].tobytes()
        assert ctx.requant_timing()[1] > 0.0
        a.free()
        b.free()
    finally:
        rec.free()
    path = tmp_path / "wide.bin"
    x.tofile(str(path))
    opened = ctx.open_file(str(path), 0, x.nbytes)                              # still streaming in when the calls are made
    try:
        st = ctx.requant_stats(opened, dtype)
        out = ctx.requantize(opened, dtype, **GAIN[dtype])
        assert out.download().tobytes() == want.tobytes()
        out.free()
        assert st["n_finite"] + st["n_nonfinite"] == x.size
    finally:
        opened.free()


# ---- statistics --------------------------------------------------------------------------------------------------------------

def check_stats(got, x, offset, count):
    """got against the contract on elements [offset, offset + count) of x: exact, or within the bounds (float32 sums)."""
    want = spec.stats(x, x.dtype, offset, count)
    assert (got["n_finite"], got["n_nonfinite"], got["max_abs"]) == (want["n_finite"], want["n_nonfinite"], want["max_abs"]), \
        (x.dtype, offset, count, got, want)
    if x.dtype == spec.INT16:
        assert (got["sum"], got["sum_sq"]) == (want["sum"], want["sum_sq"]), (offset, count, got, want)
    else:
        b_sum, b_sq = spec.bounds(want, count)
        print("float32 window (%d, %d): |sum - fsum| = %.3g (bound %.3g), |sum_sq - fsum| = %.3g (bound %.3g)"
              % (offset, count, abs(got["sum"] - want["sum"]), b_sum, abs(got["sum_sq"] - want["sum_sq"]), b_sq))
        assert abs(got["sum"] - want["sum"]) <= b_sum, (offset, count, got, want)
        assert abs(got["sum_sq"] - want["sum_sq"]) <= b_sq, (offset, count, got, want)


def windows(n, tile):
    w = [(0, n), (n, 0), (0, 0), (1, 1), (3, tile + 2), (5, 2 * tile + 7), (7, 1001), (1, n - 1), (0, n - 1), (8, 8), (9, 7)]
    return [(o, c) for o, c in w if c >= 0 and o + c <= n]


@pytest.mark.parametrize("dtype", DTYPES)
def test_statistics_on_every_length_and_window(ctx, tile, dtype):
    rng = np.random.default_rng(30)
    for ln in lengths(tile):
        x = sample_record(rng, dtype, ln)
        rec = up(ctx, x)
        try:
            check_stats(ctx.requant_stats(rec, dtype), x, 0, ln)
            assert ln == 0 or ctx.requant_timing()[0] > 0.0
            for o, c in windows(ln, tile):
                got = ctx.requant_stats(rec, dtype, o, c)
                check_stats(got, x, o, c)
                again = ctx.requant_stats(rec, dtype, o, c)
                assert all(np.float64(got[k]).tobytes() == np.float64(again[k]).tobytes() for k in got), (o, c)
        finally:
            rec.free()


def test_int16_statistics_at_the_largest_sum(ctx):
    x = np.full(1 << 20, -32768, dtype="<i2")
    rec = up(ctx, x)
    try:
        got = ctx.requant_stats(rec, "int16")
        assert got == dict(n_finite=1 << 20, n_nonfinite=0, max_abs=32768.0, sum=-(2.0 ** 35), sum_sq=2.0 ** 50)
        check_stats(ctx.requant_stats(rec, "int16", 3, (1 << 20) - 8), x, 3, (1 << 20) - 8)
    finally:
        rec.free()
    # sums whose exact value is not a double: the single conversion rounds it as float(int) does
    x = np.random.default_rng(31).integers(-32768, 32768, (1 << 20) + 3).astype("<i2")
    rec = up(ctx, x)
    try:
        check_stats(ctx.requant_stats(rec, "int16"), x, 0, x.size)
    finally:
        rec.free()


def test_float32_statistics_on_patterns_and_on_nan_alone(ctx):
    patterns = np.random.default_rng(3).integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype("<u4").view("<f4")
    rec = up(ctx, patterns)
    try:
        for o, c in ((0, patterns.size), (1, patterns.size - 2), (12345, 54321)):
            got = ctx.requant_stats(rec, "float32", o, c)
            check_stats(got, patterns, o, c)
            again = ctx.requant_stats(rec, "float32", o, c)
            assert all(np.float64(got[k]).tobytes() == np.float64(again[k]).tobytes() for k in got)
    finally:
        rec.free()
    # denormals count with their value; a window of NaN and infinities alone has no finite element
    x = np.concatenate([np.full(1000, 1e-41, dtype="<f4"), np.full(777, np.nan, dtype="<f4"),
                        np.array([np.inf, -np.inf], dtype="<f4"), np.full(5, -3e-39, dtype="<f4")])
    rec = up(ctx, x)
    try:
        check_stats(ctx.requant_stats(rec, "float32", 0, 1000), x, 0, 1000)
        assert ctx.requant_stats(rec, "float32", 0, 1000)["sum"] > 0.0
        got = ctx.requant_stats(rec, "float32", 1000, 779)
        assert got == dict(n_finite=0, n_nonfinite=779, max_abs=0.0, sum=0.0, sum_sq=0.0)
        assert pkg()._native.requant_gain(got, "float32", 12.0)[2] == np.float32(1.0)
        check_stats(ctx.requant_stats(rec, "float32"), x, 0, x.size)
    finally:
        rec.free()


def test_refusals_on_the_device(ctx):
    """The two refusals that look at the record, and the others once more with a record and a context in hand."""
    n = pkg()._native
    rec = ctx.upload(np.zeros(1000, dtype=np.int8))
    odd = ctx.upload(np.zeros(1002, dtype=np.int8))
    odder = ctx.upload(np.zeros(1001, dtype=np.int8))
    try:
        for r, dt in ((odder, "int16"), (odder, "float32"), (odd, "float32")):
            for call in (lambda: ctx.requantize(r, dt), lambda: ctx.requant_stats(r, dt, 0, 1)):
                with pytest.raises(n.SgxError) as e:
                    call()
                assert e.value.code == n.SGX_E_ARG and "whole" in str(e.value) and "bytes" in str(e.value)
        for dt, w in (("int16", 2), ("float32", 4)):
            for o, c in ((1000 // w + 1, 0), (0, 1000 // w + 1), (1000 // w, 1), (7, 1000 // w - 6)):
                with pytest.raises(n.SgxError) as e:
                    ctx.requant_stats(rec, dt, o, c)
                assert e.value.code == n.SGX_E_ARG and "window" in str(e.value) and "count" in str(e.value), (dt, o, c)
            assert ctx.requant_stats(rec, dt, 1000 // w, 0)["n_finite"] == 0
        for kw, word in ((dict(mult=0), "mult"), (dict(mult=32768), "mult"), (dict(mult=1, shift=31), "shift"),
                         (dict(mult=1, shift=-1), "shift")):
            with pytest.raises(n.SgxError) as e:
                ctx.requantize(rec, "int16", **kw)
            assert e.value.code == n.SGX_E_ARG and word in str(e.value)
        for scale in (0.0, float("nan"), float("inf"), 2.0 ** 101, 2.0 ** -101, -1.0):
            with pytest.raises(n.SgxError) as e:
                ctx.requantize(rec, "float32", scale=scale)
            assert e.value.code == n.SGX_E_ARG and "scale" in str(e.value)
        out = C.c_void_p()
        f = n.lib().sgx_if_requantize
        assert f(ctx._h, rec._h, n.DT_INT8, 1, 0, 1.0, C.byref(out), None) == n.SGX_E_ARG and "data_type" in n.last_error()
        assert f(ctx._h, None, n.DT_INT16, 1, 0, 1.0, C.byref(out), None) == n.SGX_E_ARG
        assert f(ctx._h, rec._h, n.DT_INT16, 1, 0, 1.0, None, None) == n.SGX_E_ARG
        assert f(None, rec._h, n.DT_INT16, 1, 0, 1.0, C.byref(out), None) == n.SGX_E_ARG
        assert n.lib().sgx_requant_stats_of(ctx._h, rec._h, n.DT_INT16, 0, 1, None) == n.SGX_E_ARG
        assert not out.value
        # no count is asked for: the call works without it
        assert f(ctx._h, rec._h, n.DT_INT16, 1, 0, 1.0, C.byref(out), None) == n.SGX_OK and out.value
        assert n.lib().sgx_if_free(ctx._h, out) == n.SGX_OK
    finally:
        odder.free()
        odd.free()
        rec.free()


# ---- end to end: scene 1 as an int16 and as a float32 capture ------------------------------------------------------------

def _record_ms():
    return TRK_MS + 4


def _same_search(a, ref):
    assert np.array_equal(a.codePhase, ref["codePhase"])
    assert np.array_equal(a.carrFreq, ref["carrFreq"])
    assert np.array_equal(np.asarray(a.internals["freqBin"]), ref["freqBin"])
    assert np.allclose(a.peakMetric, ref["peakMetric"], rtol=1e-9, atol=0)


@pytest.mark.parametrize("skip_pairs", [0, 1000])
@pytest.mark.parametrize("dtype", DTYPES)
def test_post_processing_of_a_wide_iq_file(tmp_path, dtype, skip_pairs):
    m = pkg()
    w = np.dtype(dtype).itemsize
    x = cases.wide_record(dtype, _record_ms())
    path = tmp_path / ("scene_%s.bin" % dtype)
    x.tofile(str(path))
    s = SCENE.settings(m, msToProcess=float(TRK_MS), dataType=dtype, iqRequantize=True,
                       skipNumberOfBytes=2 * w * skip_pairs)
    skip = 2 * skip_pairs                                                       # samples of the prepared record
    acq, trk, nav = s.postProcessing(str(path))
    assert nav is None or nav._solutions is None                               # 300 ms carry no subframe
    info = dict(s.lastRequant)
    count = info["n_finite"] + info["n_nonfinite"]                             # the components that were read
    assert info["n_nonfinite"] == 0 and skip + TRK_MS * SCENE.samples_per_code < count <= x.size
    assert s.iqRecord and s.samplingFreq == SCENE.fs_c and s.skipNumberOfBytes == 2 * w * skip_pairs   # left alone
    assert acq.settings.skipNumberOfBytes == skip and acq.settings.dataType == 'int8' and not acq.settings.iqRecord
    # the statistics the run took, and the gain it made of them
    check_stats(info, x, 0, count)
    mult, shift, scale = spec.gain(info["n_finite"], info["sum_sq"], s.iqTargetRms)
    if dtype == "int16":
        assert (info["mult"], info["shift"]) == (mult, shift)
    else:
        assert np.float32(info["scale"]).tobytes() == np.float32(scale).tobytes()
    y8 = spec.quantise(x[:count], x.dtype, mult, shift, scale)
    assert info["clipped"] == spec.clipped_share(y8)
    assert abs(info["rms"] - math.sqrt(info["sum_sq"] / count)) <= 1e-12 * info["rms"]
    want = cases.contract_record(x[:count], mult, shift, scale)
    # the prepared record is the contracts', byte for byte; a second preparation takes the same statistics, bit for bit
    with s._prepared_record(str(path), 0, count) as rec:
        assert rec.download().tobytes() == want.tobytes()
    assert all(np.array_equal(np.float64(s.lastRequant[k]), np.float64(info[k])) for k in info)
    # acquisition and tracking against the oracle on that record
    n = SCENE.samples_per_code
    o = SCENE.oracle_settings(msToProcess=float(TRK_MS), skipNumberOfBytes=skip)
    ref = orc.acquire(o, want[skip:skip + 11 * n])
    _same_search(acq, ref)
    assert sorted(np.flatnonzero(acq.carrFreq) + 1) == sorted(SCENE.prns)
    chans = orc.pre_run(o, ref)
    assert np.array_equal(acq.channels.PRN, chans["PRN"]) and np.count_nonzero(acq.channels.PRN) == len(SCENE.prns)
    same_tracking(trk, orc.stack_series(orc.track(o, chans, want)), len(SCENE.prns), TRK_MS)
