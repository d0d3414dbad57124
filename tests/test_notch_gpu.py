"""Interference excision on the GPU (sgx_if_filter, csrc/sgx_filter.hip; Settings.mitigate): the filter against the numpy
contract of tests/notch_spec.py byte for byte, then acquisition and tracking on the mitigated record against the oracle on
the contract-filtered record, by the bars of tests/test_gpu_parity.py.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import notch_cases as cases
import notch_spec as spec
from conftest import pkg
from oracle import softgnss_oracle as orc
from record_stage import full_scale, same_tracking

pytestmark = pytest.mark.gpu

TRK_MS = 100


@pytest.fixture(scope="module")
def ctx():
    m = pkg()
    return m.engine.get_context(m.Settings(), 0)


def random_taps(rng, L, total):
    """int16 taps reaching +-32512 whose sum of magnitudes stays within `total` (< 2^24: the accumulator bound)."""
    h = np.zeros(L, dtype=np.int64)
    k = max(1, min(L, total // spec.MAX_TAP))
    pos = rng.choice(L, size=k, replace=False)
    h[pos] = rng.integers(-spec.MAX_TAP, spec.MAX_TAP + 1, k)
    h[pos[0]] = spec.MAX_TAP
    if k > 1:
        h[pos[1]] = -spec.MAX_TAP
    rest = np.setdiff1d(np.arange(L), pos)
    room = total - int(np.abs(h).sum())
    if rest.size and room > rest.size:
        h[rest] = rng.integers(-(room // rest.size), room // rest.size + 1, rest.size)
    assert 128 * int(np.abs(h).sum()) < 2 ** 31
    return h.astype(np.int16)


def fine_taps(rng, L, S):
    """Taps scaled so that the outputs spread over -127 .. 127 instead of sitting on the rails: a wrong sum shows."""
    sigma = 40.0 * (1 << S) / (74.0 * np.sqrt(L))
    if sigma >= 1.0:
        return np.clip(np.rint(rng.normal(0.0, sigma, L)), -spec.MAX_TAP, spec.MAX_TAP).astype(np.int16)
    h = np.zeros(L, dtype=np.int16)
    pos = rng.choice(L, size=min(L, 4), replace=False)
    h[pos] = rng.choice([-1, 1], size=pos.size)
    return h


def run(ctx, x, h, S):
    rec = ctx.upload(x)
    try:
        out = ctx.filter_record(rec, h, S)
        try:
            assert len(out) == x.size
            return out.download()
        finally:
            out.free()
    finally:
        rec.free()


@pytest.mark.parametrize("S", [0, 14])
@pytest.mark.parametrize("L", [1, 3, 255, 1025, 4095])
def test_random_filters_equal_the_contract(ctx, L, S):
    rng = np.random.default_rng(1000 * L + S)
    x = full_scale(rng, 100003)
    # S = 14: sums of the order 2^14 .. 2^21, outputs spread over the range; S = 0: nearly every output on a rail
    h = random_taps(rng, L, (1 << 24) - 1 if L > 600 else 40000 * L)
    want = spec.apply(x, h, S)
    got = run(ctx, x, h, S)
    assert got.tobytes() == want.tobytes(), "first difference at sample %d" % int(np.flatnonzero(got != want)[0])
    # the same with taps of a size that keeps most outputs off the rails
    h = fine_taps(rng, L, S)
    want = spec.apply(x, h, S)
    assert np.count_nonzero(np.abs(want.astype(int)) < 127) > x.size // 2
    got = run(ctx, x, h, S)
    assert got.tobytes() == want.tobytes(), "first difference at sample %d" % int(np.flatnonzero(got != want)[0])


def test_record_shorter_than_the_filter(ctx):
    rng = np.random.default_rng(5)
    x = full_scale(rng, 100)
    h = random_taps(rng, 1025, (1 << 24) - 1)
    for S in (0, 14):
        assert run(ctx, x, h, S).tobytes() == spec.apply(x, h, S).tobytes()
    assert run(ctx, x[:1], h, 14).tobytes() == spec.apply(x[:1], h, 14).tobytes()
    assert run(ctx, x[:0], h, 14).size == 0


def test_saturation_at_both_rails_and_identity(ctx):
    rng = np.random.default_rng(6)
    x = full_scale(rng, 100003)
    for L in (1, 255, 4095):
        for S in (0, 14):
            ident = np.zeros(L, dtype=np.int16)
            ident[(L - 1) // 2] = 1 << S
            assert run(ctx, x, ident, S).tobytes() == np.clip(x, -127, 127).tobytes(), (L, S)
    gain = np.zeros(255, dtype=np.int16)
    gain[127] = 3 << 12                                  # y = clip(3 x)
    got = run(ctx, x, gain, 12)
    assert got.tobytes() == spec.apply(x, gain, 12).tobytes()
    assert got.min() == -127 and got.max() == 127 and np.count_nonzero(np.abs(got.astype(int)) == 127) > x.size // 2
    # the accumulator's ends: every product at full scale, sum = +-(2^31 - 128) * ... within int32 by the contract's bound
    full = np.full(4095, 4097, dtype=np.int16)           # sum|h| = 2^24 - 1
    flat = np.full(10000, -128, dtype=np.int8)
    for S in (0, 24, 30):
        assert run(ctx, flat, full, S).tobytes() == spec.apply(flat, full, S).tobytes(), S
        assert run(ctx, flat, -full, S).tobytes() == spec.apply(flat, -full, S).tobytes(), S


def test_many_workgroups_and_tile_seams(ctx):
    rng = np.random.default_rng(8)
    n = (1 << 21) + 17
    x = full_scale(rng, n)
    h = random_taps(rng, 1025, (1 << 24) - 1)
    want = spec.apply(x, h, 14)
    rec = ctx.upload(x)
    try:
        a = ctx.filter_record(rec, h, 14)
        b = ctx.filter_record(rec, h, 14)
        ga, gb = a.download(), b.download()
        a.free()
        b.free()
        assert rec.download().tobytes() == x.tobytes()   # the input is left alone
    finally:
        rec.free()
    assert ga.tobytes() == want.tobytes(), "first difference at sample %d" % int(np.flatnonzero(ga != want)[0])
    assert ga.tobytes() == gb.tobytes()
    assert ctx.filter_timing() > 0.0


@pytest.mark.parametrize("L", [3, 255])
def test_lengths_around_a_tile_seam(ctx, L):
    """The load and store guards where they can be wrong: a record that ends one sample before, on and one sample after a
    16-byte group and a workgroup's tile (_native.iq_tile(): the tile the two stages share)."""
    tile = pkg()._native.iq_tile()
    rng = np.random.default_rng(2000 + L)
    for h in (fine_taps(rng, L, 14), random_taps(rng, L, 40000 * L)):
        for n in (15, 16, 17, tile - 1, tile, tile + 1, 3 * tile + 1):
            x = full_scale(rng, n)
            want = spec.apply(x, h, 14)
            got = run(ctx, x, h, 14)
            assert got.tobytes() == want.tobytes(), \
                "N = %d: first difference at sample %d" % (n, int(np.flatnonzero(got != want)[0]))


def test_refusals_on_the_device(ctx):
    m = pkg()
    n = m._native
    rec = ctx.upload(np.zeros(1000, dtype=np.int8))
    try:
        for h, S in ((np.zeros(4, dtype=np.int16), 14), (np.zeros(3, dtype=np.int16), 31), (np.zeros(3, dtype=np.int16), -1),
                     (np.full(3, 32513, dtype=np.int16), 0), (np.full(4095, 4098, dtype=np.int16), 0)):
            with pytest.raises(n.SgxError) as e:
                ctx.filter_record(rec, h, S)
            assert e.value.code == n.SGX_E_ARG
        out = C.c_void_p()
        h = np.zeros(3, dtype=np.int16)
        assert n.lib().sgx_if_filter(ctx._h, None, n._ptr(h), 3, 0, C.byref(out)) == n.SGX_E_ARG
        assert n.lib().sgx_if_filter(ctx._h, rec._h, n._ptr(h), 3, 0, None) == n.SGX_E_ARG
    finally:
        rec.free()


def _settings(m):
    s = m.Settings()
    s.msToProcess = float(TRK_MS)
    return s


@pytest.fixture(scope="module")
def mitigated():
    """The jammed scene on the GPU through Settings.mitigate, and the contract's own mitigation of it on the host."""
    m = pkg()
    s = _settings(m)
    c = m.engine.get_context(s, 0)
    rec = c.upload(cases.jammed(TRK_MS))
    new, lines = s.mitigate(rec)
    want, want_lines, taps, shift = cases.contract_mitigated(TRK_MS)
    yield m, s, c, rec, new, lines, want, want_lines
    if new is not rec:
        new.free()
    rec.free()


def test_mitigate_finds_the_one_line_and_filters_as_the_contract(mitigated):
    m, s, c, rec, new, lines, want, want_lines = mitigated
    assert len(lines) == 1 and new is not rec and len(new) == len(rec)
    f_bin = s.samplingFreq / 16384.0
    assert abs(lines[0][0] - (s.IF + cases.CW_OFFSET_HZ)) <= f_bin
    # the GPU's Welch spectrum differs from numpy's in the last bits: the same bin and width must come out of it
    assert lines == want_lines
    assert new.download().tobytes() == want.tobytes()


def test_acquisition_on_the_mitigated_record(mitigated):
    m, s, c, rec, new, lines, want, _ = mitigated
    n = s.samplesPerCode
    os_ = orc.OracleSettings(msToProcess=float(TRK_MS))
    ref = orc.acquire(os_, want[:11 * n])
    a = m.AcquisitionResult(s, device=0)
    a.acquire(m.DeviceSignal(new, 0, 11 * n))
    assert np.array_equal(a.codePhase, ref["codePhase"])
    assert np.array_equal(a.carrFreq, ref["carrFreq"])
    assert np.allclose(a.peakMetric, ref["peakMetric"], rtol=1e-9, atol=0)
    got = c.acquire(new, 0, 11 * n, np.arange(32))
    det = ref["carrFreq"] != 0
    assert np.array_equal(got["freqBin"][det], np.asarray(ref["freqBin"])[det])
    assert sorted(np.flatnonzero(a.carrFreq) + 1) == list(cases.PRESENT)
    for p in cases.ABSENT:
        assert a.carrFreq[p - 1] == 0
    # ... and without the stage the same search loses satellites to the jammer
    b = m.AcquisitionResult(s, device=0)
    b.acquire(m.DeviceSignal(rec, 0, 11 * n))
    assert np.count_nonzero(b.carrFreq) <= 6


def test_tracking_on_the_mitigated_record(mitigated):
    m, s, c, rec, new, lines, want, _ = mitigated
    n = s.samplesPerCode
    os_ = orc.OracleSettings(msToProcess=float(TRK_MS))
    ref = orc.acquire(os_, want[:11 * n])
    chans_ref = orc.pre_run(os_, ref)
    a = m.AcquisitionResult(s, device=0)
    a.acquire(m.DeviceSignal(new, 0, 11 * n))
    a.preRun()
    assert np.array_equal(a.channels.PRN, chans_ref["PRN"]) and np.count_nonzero(a.channels.PRN) == 8
    t = m.TrackingResult(a, device=0)
    t.track(m.DeviceFile(new))
    series = orc.stack_series(orc.track(os_, chans_ref, want))
    same_tracking(t, series, 8, TRK_MS)
    assert np.max(np.abs(t.series[:, 1] - series[:, 1])) < 1e-6        # codeFreq, Hz


def test_no_line_returns_the_same_record():
    m = pkg()
    s = _settings(m)
    c = m.engine.get_context(s, 0)
    rec = c.synth(m.synth.Scene.default(), m.synth.record_length(s.samplesPerCode, 10))
    try:
        new, lines = s.mitigate(rec)
        assert lines == [] and new is rec
    finally:
        rec.free()
