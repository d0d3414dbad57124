"""The I/Q front stage on the GPU (sgx_if_from_iq, csrc/sgx_iq.hip; Settings.convertIQ, postProcessing with iqRecord): the
converter against the numpy contract of tests/iq_spec.py byte for byte, then acquisition and tracking on the converted
record against the oracle on the contract's record, by the bars of tests/test_gpu_parity.py.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import iq_cases as cases
import iq_spec as spec
from conftest import pkg
from oracle import softgnss_oracle as orc
from record_stage import full_scale, same_tracking

pytestmark = pytest.mark.gpu

TRK_MS = 300
SCENE = cases.SCENES[0]
FLAGS = (0, spec.Q_FIRST, spec.OFFSET_BINARY, spec.Q_FIRST | spec.OFFSET_BINARY)


@pytest.fixture(scope="module")
def ctx():
    m = pkg()
    return m.engine.get_context(m.Settings(), 0)


@pytest.fixture(scope="module")
def tile():
    return pkg()._native.iq_tile()


def lengths(tile):
    return [2, 4, 6, 254, 510, 4098, 65538, tile - 2, tile, tile + 2, 3 * tile + 2]


def dense_taps(rng, L, S):
    """Random taps without a zero among them, of a size that spreads the outputs over -127 .. 127 for this shift."""
    sigma = max(2.0, 40.0 * (1 << S) / (74.0 * np.sqrt(L / 2.0)))
    h = np.clip(np.rint(rng.normal(0.0, sigma, L)), -spec.MAX_TAP, spec.MAX_TAP).astype(np.int16)
    h[h == 0] = 1
    return h


def run(ctx, b, h, S, flags=0):
    rec = ctx.upload(np.ascontiguousarray(b).view(np.int8))
    try:
        out = ctx.iq_to_if(rec, h, S, q_first=bool(flags & spec.Q_FIRST), offset_binary=bool(flags & spec.OFFSET_BINARY))
        try:
            assert len(out) == b.size
            return out.download()
        finally:
            out.free()
    finally:
        rec.free()


def same(ctx, b, h, S, flags=0):
    want = spec.convert(b, h, S, flags)
    got = run(ctx, b, h, S, flags)
    assert got.tobytes() == want.tobytes(), \
        "N = %d, L = %d, S = %d, flags = %d: first difference at sample %d" % (b.size, len(h), S, flags,
                                                                               int(np.flatnonzero(got != want)[0]))
    return want


def test_single_tap_and_hold(ctx, tile):
    """[1], S = 0: y = I, 0, -I, 0 (zero-stuffing leaves the half-period instants empty); [0, 1, 1]: y = I, -Q, -I, Q."""
    rng = np.random.default_rng(1)
    for n in lengths(tile):
        b = full_scale(rng, n)
        I, Q = np.clip(b[0::2].astype(np.int64), -127, 127), np.clip(b[1::2].astype(np.int64), -127, 127)
        sign = np.where(np.arange(n // 2) % 2 == 0, 1, -1)
        y = same(ctx, b, np.array([1], dtype=np.int16), 0)
        assert np.array_equal(y[0::2], sign * I) and not y[1::2].any()
        y = same(ctx, b, np.array([0, 1, 1], dtype=np.int16), 0)
        assert np.array_equal(y[0::2], sign * I) and np.array_equal(y[1::2], -sign * Q)


@pytest.mark.parametrize("S", [0, 7, 14])
@pytest.mark.parametrize("L", [3, 5, 63, 255])
def test_dense_random_taps_equal_the_contract(ctx, tile, L, S):
    rng = np.random.default_rng(1000 * L + S)
    h = dense_taps(rng, L, S)
    assert np.all(h != 0)
    off_rails = 0
    for n in lengths(tile):
        want = same(ctx, full_scale(rng, n), h, S)
        off_rails += np.count_nonzero(np.abs(want.astype(int)) < 127)
    if S:                                            # (S = 0: a sum of products of full-scale bytes is mostly on a rail)
        assert off_rails > sum(lengths(tile)) // 2   # a wrong sum shows: the outputs are not sitting on the rails


@pytest.mark.parametrize("L", [3, 5, 63, 255])
def test_records_shorter_than_the_filter(ctx, L):
    rng = np.random.default_rng(50 + L)
    h = dense_taps(rng, L, 7)
    for n in sorted({0, 2, 4, (L - 1) // 2 & ~1, L - 1, L + 1}):
        if n == 0:
            assert run(ctx, np.zeros(0, dtype=np.int8), h, 7).size == 0
        else:
            same(ctx, full_scale(rng, n), h, 7)


@pytest.mark.parametrize("S", [30, 16])
def test_accumulator_and_clip_at_their_limits(ctx, tile, S):
    """Every tap at +-32 512 over the longest filter the accumulator bound admits, on full-scale input."""
    L = spec.MAX_TAPS
    assert 128 * (L * spec.MAX_TAP) < 2 ** 31      # the longest filter there is stays within the accumulator bound
    rng = np.random.default_rng(60 + S)
    n = tile + 2
    k = np.arange(n)
    for h in (np.full(L, spec.MAX_TAP), np.full(L, -spec.MAX_TAP), np.where(np.arange(L) % 4 < 2, spec.MAX_TAP, -spec.MAX_TAP),
              rng.choice([-spec.MAX_TAP, spec.MAX_TAP], L)):
        h = h.astype(np.int16)
        for b in (np.full(n, -128), np.full(n, 127), np.where(k % 2 == 0, -128, 127), np.where(k % 4 < 2, -128, 127),
                  rng.choice([-128, -127, 127], n)):
            want = same(ctx, b.astype(np.int8), h, S)
        assert S == 30 or (want.min() == -127 and want.max() == 127)
    # the sum itself at the accumulator's end: all products 128 * 32 512 of one sign
    b = np.full(n, -128, dtype=np.int8)
    h = np.full(L, spec.MAX_TAP, dtype=np.int16)
    assert np.abs(spec.convert(b, h, 0).astype(int)).max() == 127
    same(ctx, b, h, 0)


@pytest.mark.parametrize("L", [31, 63])
def test_designed_taps_equal_the_contract(ctx, tile, L):
    m = pkg()
    h, S = m._native.iq_design(L)
    rng = np.random.default_rng(70 + L)
    for n in lengths(tile):
        same(ctx, full_scale(rng, n), h, S)
        same(ctx, np.clip(np.rint(rng.normal(0.0, 14.0, n)), -128, 127).astype(np.int8), h, S)


@pytest.mark.parametrize("flags", FLAGS)
def test_flags(ctx, tile, flags):
    rng = np.random.default_rng(80 + flags)
    m = pkg()
    for h, S in ((dense_taps(rng, 63, 7), 7), m._native.iq_design(63), (np.array([0, 1, 1], dtype=np.int16), 0)):
        for n in (tile + 2, 3 * tile + 2, 510):
            b = full_scale(rng, n)
            want = same(ctx, b, h, S, flags)
            if flags & spec.OFFSET_BINARY:           # ... equals the int8 path on b ^ 0x80
                plain = run(ctx, (b.view(np.uint8) ^ 0x80).view(np.int8), h, S, flags & ~spec.OFFSET_BINARY)
                assert plain.tobytes() == want.tobytes()
            if flags & spec.Q_FIRST:                 # ... equals the I-first path on the swapped pairs
                plain = run(ctx, b.reshape(-1, 2)[:, ::-1].ravel(), h, S, flags & ~spec.Q_FIRST)
                assert plain.tobytes() == want.tobytes()


def test_record_behaviour(ctx, tile, tmp_path):
    m = pkg()
    n = m._native
    rng = np.random.default_rng(90)
    b = full_scale(rng, 3 * tile + 2)
    h, S = n.iq_design(63)
    want = spec.convert(b, h, S)
    rec = ctx.upload(b)
    try:
        a = ctx.iq_to_if(rec, h, S)
        again = ctx.iq_to_if(rec, h, S)
        assert rec.download().tobytes() == b.tobytes()                       # the input is left alone
        ln = C.c_size_t(0)
        assert n.lib().sgx_if_length(a._h, C.byref(ln)) == n.SGX_OK and ln.value == b.size == len(a)
        assert a.download().tobytes() == want.tobytes() and again.download().tobytes() == want.tobytes()
        assert a.download(tile - 3, 11).tobytes() == want[tile - 3:tile + 8].tobytes()
        assert ctx.iq_timing() > 0.0
        # the output is an ordinary record: it goes through the converter again (read as if it were I/Q) and is freed
        twice = ctx.iq_to_if(a, h, S)
        assert twice.download().tobytes() == spec.convert(want, h, S).tobytes()
        twice.free()
        a.free()
        again.free()
        assert not a._h
    finally:
        rec.free()
    path = tmp_path / "iq.bin"
    b.tofile(str(path))
    opened = ctx.open_file(str(path), 0, b.size)                             # still streaming in when the call is made
    try:
        out = ctx.iq_to_if(opened, h, S)
        assert out.download().tobytes() == want.tobytes()
        out.free()
    finally:
        opened.free()


def test_refusals_on_the_device(ctx):
    m = pkg()
    n = m._native
    good, S = n.iq_design(63)
    rec = ctx.upload(np.zeros(1000, dtype=np.int8))
    odd = ctx.upload(np.zeros(1001, dtype=np.int8))
    try:
        for h, s in ((np.zeros(4, dtype=np.int16), 14), (np.zeros(257, dtype=np.int16), 14), (np.zeros(3, dtype=np.int16), 31),
                     (np.zeros(3, dtype=np.int16), -1), (np.full(3, 32513, dtype=np.int16), 0)):
            with pytest.raises(n.SgxError) as e:
                ctx.iq_to_if(rec, h, s)
            assert e.value.code == n.SGX_E_ARG
        with pytest.raises(n.SgxError) as e:
            ctx.iq_to_if(odd, good, S)
        assert e.value.code == n.SGX_E_ARG and "pairs" in str(e.value)
        out = C.c_void_p()
        f = n.lib().sgx_if_from_iq
        assert f(ctx._h, rec._h, n._ptr(good), 63, S, 4, C.byref(out)) == n.SGX_E_ARG and "flags" in n.last_error()
        assert f(ctx._h, None, n._ptr(good), 63, S, 0, C.byref(out)) == n.SGX_E_ARG
        assert f(ctx._h, rec._h, None, 63, S, 0, C.byref(out)) == n.SGX_E_ARG
        assert f(ctx._h, rec._h, n._ptr(good), 63, S, 0, None) == n.SGX_E_ARG
        assert f(None, rec._h, n._ptr(good), 63, S, 0, C.byref(out)) == n.SGX_E_ARG
        assert not out.value
    finally:
        odd.free()
        rec.free()


# ---- end to end: scene 1 -------------------------------------------------------------------------------------------------

def _record_ms():
    """Code periods of the file: what acquisition and TRK_MS blocks behind the last code phase need."""
    return TRK_MS + 4


@pytest.fixture(scope="module")
def reference():
    """The contract's record of scene 1 under the oracle: acquisition, channels, TRK_MS ms of tracking."""
    want = cases.contract_record(SCENE, _record_ms())
    o = SCENE.oracle_settings(msToProcess=float(TRK_MS))
    acq = cases.contract_acquisition(SCENE, _record_ms())
    chans = orc.pre_run(o, acq)
    series = orc.stack_series(orc.track(o, chans, want))
    return want, o, acq, chans, series


def _same_search(a, ref):
    assert np.array_equal(a.codePhase, ref["codePhase"])
    assert np.array_equal(a.carrFreq, ref["carrFreq"])
    assert np.array_equal(np.asarray(a.internals["freqBin"]), ref["freqBin"])
    assert np.allclose(a.peakMetric, ref["peakMetric"], rtol=1e-9, atol=0)


def _same_tracking(t, series):
    same_tracking(t, series, len(SCENE.prns), TRK_MS)


def test_scene_converts_acquires_and_tracks_as_the_oracle(reference):
    want, o, ref, chans_ref, series = reference
    m = pkg()
    s = SCENE.settings(m, msToProcess=float(TRK_MS))
    real = s.realEquivalent()
    n = real.samplesPerCode
    assert n == SCENE.samples_per_code and (real.samplingFreq, real.IF) == (o.samplingFreq, o.IF)
    c = m.engine.get_context(real, 0)
    raw = c.upload(cases.iq_record(SCENE, _record_ms()))
    rec = s.convertIQ(raw)
    try:
        assert rec.download().tobytes() == want.tobytes()
        a = m.AcquisitionResult(real, device=0)
        a.acquire(m.DeviceSignal(rec, 0, 11 * n))
        _same_search(a, ref)
        assert sorted(np.flatnonzero(a.carrFreq) + 1) == sorted(SCENE.prns)
        a.preRun()
        assert np.array_equal(a.channels.PRN, chans_ref["PRN"]) and np.count_nonzero(a.channels.PRN) == len(SCENE.prns)
        t = m.TrackingResult(a, device=0)
        t.track(m.DeviceFile(rec))
        _same_tracking(t, series)
        # the loops hold: the prompt arm carries the signal, at the amplitude the scene gave it
        for ch in range(series.shape[0]):
            i = SCENE.prns.index(int(a.channels.PRN[ch]))
            prompt = np.sqrt(np.mean(t.series[ch, 3, 100:] ** 2))
            assert prompt > 0.5 * SCENE.amplitude[i] * n / 2.0, (ch, prompt)
    finally:
        rec.free()
        raw.free()


def test_post_processing_of_an_iq_file(reference, tmp_path):
    want, o, ref, chans_ref, series = reference
    m = pkg()
    path = tmp_path / "scene_iq.bin"
    cases.iq_record(SCENE, _record_ms()).tofile(str(path))
    s = SCENE.settings(m, msToProcess=float(TRK_MS))
    acq, trk, nav = s.postProcessing(str(path))
    assert nav is None or nav._solutions is None                             # 300 ms carry no subframe
    assert acq.settings.samplingFreq == o.samplingFreq and acq.settings.IF == o.IF and not acq.settings.iqRecord
    assert s.iqRecord and s.samplingFreq == SCENE.fs_c                       # the caller's settings are left alone
    _same_search(acq, ref)
    assert np.array_equal(acq.channels.PRN, chans_ref["PRN"])
    _same_tracking(trk, series)
    # offset binary, Q first: the same file as an RTL-SDR with swapped channels would have written it
    u8 = (cases.iq_record(SCENE, _record_ms()).view(np.uint8) ^ 0x80).reshape(-1, 2)[:, ::-1].ravel()
    u8.tofile(str(path))
    s = SCENE.settings(m, msToProcess=float(TRK_MS), dataType='uint8', iqQFirst=True)
    acq2, trk2, _ = s.postProcessing(str(path))
    _same_search(acq2, ref)
    _same_tracking(trk2, series)
