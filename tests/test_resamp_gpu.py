"""The resampling stage on the GPU (sgx_if_resample, csrc/sgx_resamp.hip; Settings.resampleRecord, postProcessing with
resampleUp): every one of the 31 pairs, the tap lengths at which phases go empty and sums reach the accumulator's bound, the
lengths at which zero padding, the last partial store and the tile seams lie, against the numpy contract of
tests/resamp_spec.py byte for byte with exact clip counts; the record's behaviour; the refusals; then the scenes of
tests/resamp_cases.py end to end against the contract's record and the oracle on it.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import resamp_cases as cases
import resamp_spec as spec
from conftest import pkg
from oracle import softgnss_oracle as orc
from record_stage import full_scale, same_tracking

pytestmark = pytest.mark.gpu

TRK_MS = cases.TRK_MS
SHIFTS = (0, 14, 30)


@pytest.fixture(scope="module")
def ctx():
    m = pkg()
    return m.engine.get_context(m.Settings(), 0)


@pytest.fixture(scope="module")
def tile():
    """Output bytes of a workgroup at L = 16; at another L a workgroup makes tile L / 16."""
    t = pkg()._native.resamp_tile()
    assert t > 0 and t % 256 == 0
    return t


def random_taps(rng, n, shift, per_output):
    """n taps whose sums - of about per_output of them each - land on both sides of the clip at this shift, inside the
    bound on sum|h|."""
    budget = (2 ** 31 - 1) // 128
    a = 100.0 * 2.0 ** shift * np.sqrt(3.0) / (74.0 * np.sqrt(max(per_output, 1)))
    a = int(min(max(a, 1.0), spec.MAX_TAP, 1.6 * budget / n))                  # (sum|h| is about n a / 2)
    h = rng.integers(-a, a + 1, n)
    assert 128 * int(np.abs(h).sum()) < 2 ** 31
    return h.astype(np.int16)


def extreme_taps(rng, n):
    """Taps at +-32512, as many as the bound 128 sum|h| < 2^31 admits, and the rest of the bound in one more."""
    budget = (2 ** 31 - 1) // 128
    h = np.zeros(n, dtype=np.int64)
    full = min(n, budget // spec.MAX_TAP)
    h[:full] = spec.MAX_TAP
    if full < n:
        h[full] = min(spec.MAX_TAP, budget - full * spec.MAX_TAP)
    h = rng.permutation(h) * rng.choice([-1, 1], n)
    assert np.abs(h).max() == spec.MAX_TAP and 128 * int(np.abs(h).sum()) < 2 ** 31
    assert n * spec.MAX_TAP <= budget or 128 * (int(np.abs(h).sum()) + 1) >= 2 ** 31      # just inside the bound
    return h.astype(np.int16)


def same(ctx, b, h, S, L, M):
    """The bytes b through the library equal the contract byte for byte; so does the clip count."""
    want, clipped = spec.resample(b, h, S, L, M)
    rec = ctx.upload(np.ascontiguousarray(b).view(np.int8))
    try:
        out = ctx.resample(rec, h, S, L, M)
        try:
            what = (L, M, h.size, S, b.size)
            assert len(out) == want.size == spec.out_length(b.size, L, M), what
            got = out.download()
            assert got.tobytes() == want.tobytes(), \
                "%r: first difference at output byte %d" % (what, int(np.flatnonzero(got != want)[0]))
            assert out.clipped == clipped, (what, out.clipped, clipped)
        finally:
            out.free()
    finally:
        rec.free()
    return want, clipped


# ---- every pair, byte for byte ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", spec.PAIRS, ids=["%d_%d" % p for p in spec.PAIRS])
def test_every_pair_byte_for_byte(ctx, tile, pair):
    """About 2 T + 37 output bytes: two tile seams at every L (a tile is T L / 16 <= T bytes), a partial last 16-byte
    group, and an input length that is no multiple of M."""
    L, M = pair
    rng = np.random.default_rng(1000 * L + M)
    n_in = -(-(2 * tile + 37) * M // L)
    # (the first length from there on that is no multiple of M and leaves a partial group; 16 / 1 makes whole groups only)
    fits = [n for n in range(n_in, n_in + 48) if (M == 1 or n % M) and (spec.out_length(n, L, M) % 16 or (L, M) == (16, 1))]
    n_in = fits[0]
    b = full_scale(rng, n_in)
    h = random_taps(rng, spec.default_taps(L), 14, 24)
    want, clipped = same(ctx, b, h, 14, L, M)
    assert want.size >= 2 * tile + 37 and (want.size % 16 or (L, M) == (16, 1)) and (M == 1 or n_in % M)
    assert 0 < clipped < want.size


@pytest.mark.parametrize("pair", [(2, 1), (16, 1), (16, 3)], ids=["2_1", "16_1", "16_3"])
def test_tap_lengths_and_shifts(ctx, tile, pair):
    """Lh = 1, L - 1 (phases with no tap at all), 2 L + 1 and 1023 at shifts 0, 14 and 30, random taps on full-scale input;
    then taps at the bound on 128 sum|h| with all -128 input: the largest sums the accumulator is promised to hold."""
    L, M = pair
    rng = np.random.default_rng(2000 * L + M)
    n_in = -(-(tile * L // 16 + 37) * M // L) + 1
    b = full_scale(rng, n_in)
    seen_clipped = seen_unclipped = 0
    for Lh in sorted(set([1, (L - 1) | 1, 2 * L + 1, 1023])):
        for S in SHIFTS:
            h = random_taps(rng, Lh, S, -(-Lh // L))
            want, clipped = same(ctx, b, h, S, L, M)
            seen_clipped += clipped > 0
            seen_unclipped += clipped < want.size
    assert seen_clipped >= 3 and seen_unclipped >= 3
    low = np.full(n_in, -128, dtype=np.int8)
    for Lh in (511, 1023):
        h = extreme_taps(rng, Lh)
        for S in SHIFTS:
            same(ctx, low, h, S, L, M)
    # one stream holds the whole bound: every L-th tap at full scale, the others zero, signs alike - the sum of that stream
    # is -128 sum|h|, just inside int32
    h = np.zeros(1023, dtype=np.int64)
    budget = (2 ** 31 - 1) // 128
    at = np.arange(0, 1023, L)
    full = min(at.size - 1, budget // spec.MAX_TAP)
    h[at[:full]] = spec.MAX_TAP
    h[at[full]] = min(spec.MAX_TAP, budget - full * spec.MAX_TAP)
    for sign in (1, -1):
        for S in (0, 30):
            want, _ = same(ctx, low, (sign * h).astype(np.int16), S, L, M)
    assert want.size


# ---- the record's behaviour ---------------------------------------------------------------------------------------------

def test_record_behaviour(ctx, tile, tmp_path):
    m = pkg()
    n = m._native
    rng = np.random.default_rng(301)
    L, M = 7, 3
    T = tile * L // 16                                                         # output bytes of a workgroup at this L
    h = random_taps(rng, spec.default_taps(L), 14, 24)
    h1 = np.array([1 << 14], dtype=np.int16)
    # N = 1, M - 1, and around one tile of output: the longest input that makes at most one tile less one, the shortest that
    # makes at least one tile plus one (ceil(N L / M) does not take every value), at three pairs
    for l2, m2 in ((L, M), (3, 2), (2, 1)):
        t2 = tile * l2 // 16
        below = max(k for k in range(t2) if spec.out_length(k, l2, m2) <= t2 - 1)
        above = min(k for k in range(t2) if spec.out_length(k, l2, m2) >= t2 + 1)
        assert t2 - 3 <= spec.out_length(below, l2, m2) <= t2 - 1 and t2 + 1 <= spec.out_length(above, l2, m2) <= t2 + 3
        for n_in in sorted(set([1, max(1, m2 - 1), below, above])):
            same(ctx, full_scale(rng, n_in), random_taps(rng, 4 * l2 + 1, 14, 4), 14, l2, m2)
    b = full_scale(rng, 3 * T * M // L // 2 + 7)
    want, clipped = spec.resample(b, h, 14, L, M)
    assert 0 < clipped < want.size
    before = (ctx.filter_timing(), ctx.iq_timing(), ctx.requant_timing(), ctx.cond_timing(), ctx.unpack_timing(),
              ctx.decim_timing())
    rec = ctx.upload(b)
    try:
        a = ctx.resample(rec, h, 14, L, M)
        assert rec.download().tobytes() == b.tobytes()                         # the input is left alone
        ln = C.c_size_t(0)
        assert n.lib().sgx_if_length(a._h, C.byref(ln)) == n.SGX_OK and ln.value == want.size == len(a)
        assert a.download().tobytes() == want.tobytes() and a.clipped == clipped
        assert a.download(T - 3, 11).tobytes() == want[T - 3:T + 8].tobytes()
        assert ctx.resamp_timing() > 0.0
        # the other timing slots are their stages'
        assert (ctx.filter_timing(), ctx.iq_timing(), ctx.requant_timing(), ctx.cond_timing(), ctx.unpack_timing(),
                ctx.decim_timing()) == before
        # a second call's count starts from zero
        w1, c1 = spec.resample(b, h1, 14, 2, 1)
        other = ctx.resample(rec, h1, 14, 2, 1)
        assert other.download().tobytes() == w1.tobytes() and other.clipped == c1
        again = ctx.resample(rec, h, 14, L, M)
        assert again.download().tobytes() == want.tobytes() and again.clipped == clipped
        # the output is an ordinary record: it goes through the stage again and is freed
        twice = ctx.resample(a, h1, 14, 3, 2)
        w2, c2 = spec.resample(want, h1, 14, 3, 2)
        assert twice.download().tobytes() == w2.tobytes() and twice.clipped == c2
        for r in (twice, again, other, a):
            r.free()
        assert not a._h
    finally:
        rec.free()
    # a record that is still streaming in is waited for
    path = tmp_path / "resamp.bin"
    big = np.tile(b, 6)
    big.tofile(str(path))
    wbig, cbig = spec.resample(big, h, 14, L, M)
    opened = ctx.open_file(str(path), 0, big.size)
    try:
        out = ctx.resample(opened, h, 14, L, M)
        assert out.download().tobytes() == wbig.tobytes() and out.clipped == cbig
        out.free()
    finally:
        opened.free()
    # the empty record: an empty record, a zero timing slot, a zero count
    empty = ctx.upload(np.zeros(0, dtype=np.int8))
    try:
        out = ctx.resample(empty, h, 14, L, M)
        assert len(out) == 0 and out.download().size == 0 and ctx.resamp_timing() == 0.0 and out.clipped == 0
        out.free()
    finally:
        empty.free()


def test_the_output_is_searched_by_acquire():
    """The resampled record of scene a under a context of its own settings: sgx_acquire finds what the oracle finds on the
    contract's record."""
    m = pkg()
    case = cases.CASES["x10_4096"]
    b = cases.file_of(case, cases.ACQ_MS)
    want, _ = cases.prepared(case, cases.ACQ_MS)
    real = case.settings(m)._prepared_settings()
    c2 = m.engine.get_context(real, 0)
    rec = c2.upload(b)
    try:
        out = c2.resample(rec, case.taps, case.shift, case.L, case.M)
        assert out.download().tobytes() == want.tobytes()
        n = real.samplesPerCode
        got = c2.acquire(out, 0, 11 * n, np.arange(32))
        ref = cases.contract_acquisition(case)
        det = np.asarray(ref["carrFreq"]) != 0
        assert np.array_equal(got["freqBin"][det], np.asarray(ref["freqBin"])[det])
        assert np.array_equal(got["codePhase"], ref["codePhase"])
        assert sorted(np.flatnonzero(got["carrFreq"]) + 1) == sorted(case.scene.prns)
        out.free()
        assert not out._h
    finally:
        rec.free()


# ---- refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device(ctx):
    """Every refusal once more with a record and a context in hand; nothing is launched: the timing slot stays as it was.
    (An output beyond one launch - 2^31 tiles of at least 8192 bytes - does not fit a device, and a record on another
    device needs a second one: those two checks are read, not run.)"""
    n = pkg()._native
    good = np.arange(-31, 32, dtype=np.int16)
    rec = ctx.upload(np.zeros(1000, dtype=np.int8))
    try:
        ok = ctx.resample(rec, good, 14, 4, 1)
        ok.free()
        t0 = ctx.resamp_timing()
        assert t0 > 0.0
        f = n.lib().sgx_if_resample
        out, cnt = C.c_void_p(), C.c_int64(-1)

        def refused(word, r=rec, taps=good, n_taps=63, shift=14, L=4, M=1, c=ctx._h, o=C.byref(out)):
            rc = f(c, None if r is None else r._h, None if taps is None else n._ptr(taps), n_taps, shift, L, M, o,
                   C.byref(cnt))
            assert rc == n.SGX_E_ARG and word in n.last_error(), (word, rc, n.last_error())
            assert not out.value and ctx.resamp_timing() == t0

        for L, M in ((1, 1), (17, 1), (4, 2), (3, 3), (2, 3), (5, 4), (4, 0), (0, 1), (6, 3)):
            refused("L / M", L=L, M=M)
        for Lh in (0, 2, 62, 1025):
            refused("n_taps", taps=np.zeros(1100, dtype=np.int16), n_taps=Lh)
        for S in (-1, 31):
            refused("shift", shift=S)
        refused("taps", taps=None)
        refused("taps", taps=np.full(63, 32513, dtype=np.int16))
        refused("sum", taps=np.full(1023, 32512, dtype=np.int16), n_taps=1023)
        refused("rec", r=None)
        refused("out", o=None)
        refused("c &&", c=None)
        # no count is asked for: the call works without it
        assert f(ctx._h, rec._h, n._ptr(good), 63, 14, 4, 1, C.byref(out), None) == n.SGX_OK and out.value
        assert n.lib().sgx_if_free(ctx._h, out) == n.SGX_OK
    finally:
        rec.free()


# ---- end to end: the scenes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("units", [0, cases.SKIP_UNITS])
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_post_processing_of_a_resampled_file(tmp_path, name, units):
    m = pkg()
    case = cases.CASES[name]
    scene = case.scene
    L, M = case.L, case.M
    ms = TRK_MS + 4
    b = cases.file_of(case, ms)
    path = tmp_path / ("%s.bin" % name)
    b.tofile(str(path))
    s = case.settings(m, msToProcess=float(TRK_MS), skipNumberOfBytes=case.skip_in(units))
    acq, trk, nav = s.postProcessing(str(path))
    assert nav is None or nav._solutions is None                               # 0.2 s carries no subframe
    info = dict(s.lastResampling)
    skip = case.skip_out(units)                                                # samples of the prepared record
    assert (s.resampleUp, s.resampleDown, s.skipNumberOfBytes) == (L, M, case.skip_in(units))        # left alone
    assert acq.settings.skipNumberOfBytes == skip and acq.settings.dataType == 'int8' and not acq.settings.resampleUp
    assert (acq.settings.samplingFreq, acq.settings.IF) == (case.fs_out, scene.f0)
    # what the run resampled: the contract's record of the head of the file it read, with the contract's clip count
    n = int(acq.settings.samplesPerCode)
    count = info["samples"]
    n_in = count * M // L                                                      # the input samples that make `count`
    assert spec.out_length(n_in, L, M) == count and skip + TRK_MS * n < count <= spec.out_length(b.size, L, M)
    want, clipped = spec.resample(b[:n_in], case.taps, case.shift, L, M)
    assert (info["up"], info["down"], info["taps"], info["fs_out"]) == (L, M, case.n_taps, case.fs_out)
    assert info["clipped"] == clipped / float(count)
    with s._prepared_record(str(path), 0, n_in * L // M) as rec:               # (ceil(that M / L) is n_in again)
        got = rec.download()
    assert got.tobytes() == want.tobytes()
    assert s.lastResampling == info
    # every satellite of the scene where the scene put it, and no other
    assert sorted(np.flatnonzero(acq.carrFreq) + 1) == sorted(scene.prns)
    for i, prn in enumerate(scene.prns):
        assert abs(acq.carrFreq[prn - 1] - case.true_carrier(i)) <= cases.CARR_TOL_HZ, prn
        off = (acq.codePhase[prn - 1] - (case.true_phase(i) - skip) + n / 2.0) % n - n / 2.0
        assert abs(off) <= cases.PHASE_TOL * L / M, (prn, off)
    # acquisition and tracking against the oracle on the downloaded bytes
    o = orc.OracleSettings(samplingFreq=case.fs_out, IF=scene.f0, numberOfChannels=len(scene.prns), msToProcess=float(TRK_MS),
                           skipNumberOfBytes=skip)
    ref = orc.acquire(o, got[skip:skip + 11 * n])
    assert np.array_equal(acq.codePhase, ref["codePhase"]) and np.array_equal(acq.carrFreq, ref["carrFreq"])
    chans = orc.pre_run(o, ref)
    assert np.array_equal(acq.channels.PRN, chans["PRN"]) and np.count_nonzero(acq.channels.PRN) == len(scene.prns)
    series = orc.stack_series(orc.track(o, chans, got))
    same_tracking(trk, series, len(scene.prns), TRK_MS)
    # the rate the stage exists for: the speculative kernel, not the per-sample one
    ctx = m.engine.get_context(acq.settings, 0)
    assert int(ctx.timing()["track_kernel"]) == 5
