"""The multi-antenna combiner on the GPU (sgx_array_stats, sgx_if_combine, csrc/sgx_array.hip; Settings.combineAntennas,
postProcessing with antennas): the statistics as exact int64 and the combined record byte for byte with exact clip counts
against the numpy contract of tests/array_spec.py, at every number of antennas the kernels are built for, both record kinds
and the lengths at which the lags, the zero padding, the last partial store and the tile seams lie; a full-scale record
whose 32-bit partial sums would wrap if they were not flushed; the records' behaviour, the refusals, an input beyond 2^32
bytes whose period hides no wrapped address; then the scenes of tests/array_cases.py end to end against the contracts'
record and the oracle on it, and a packed four-antenna file.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import array_cases as cases
import array_spec as spec
import big_array
import big_record as big
import unpack_spec
from conftest import pkg
from oracle import softgnss_oracle as orc
from record_stage import same_tracking

pytestmark = pytest.mark.gpu

TRK_MS = cases.TRK_MS
SHIFTS = (0, 12, 30)
ANTENNAS = (2, 3, 4, 8)


def taps_of(A):
    return (1, 3, 15) if A <= 4 else (1, 3, 7)


@pytest.fixture(scope="module")
def ctx():
    m = pkg()
    return m.engine.get_context(m.Settings(), 0)


@pytest.fixture(scope="module")
def pool():
    """All 256 byte values, over and over in random order: every input longer than a few hundred bytes holds them all."""
    n = pkg()._native
    rng = np.random.default_rng(200)
    need = 16 * (3 * max(n.array_stats_tile(), n.combine_tile()) + 5) + 512
    return np.concatenate([rng.permutation(256) for _ in range(need // 256 + 2)]).astype(np.uint8)


def lengths(K, T):
    # (3 T + 5: a tile in the middle whose image lies inside the record whole - the kernels' unguarded loads)
    return sorted(set([0, 1, K - 1, K, K + 1, T - 1, T, T + 1, 2 * T + 5, 3 * T + 5]))


def random_taps(rng, A, K, lanes, shift):
    """Tap components whose sums land on both sides of the clip at this shift, inside the bound on sum|h|."""
    n = A * K * lanes
    budget = (2 ** 31 - 1) // 128
    a = 100.0 * 2.0 ** shift * np.sqrt(3.0) / (74.0 * np.sqrt(n))
    a = int(min(max(a, 1.0), spec.MAX_TAP, 1.6 * budget / n))                  # (sum|h| is about n a / 2)
    h = rng.integers(-a, a + 1, n)
    assert 128 * int(np.abs(h).sum()) < 2 ** 31
    return h.astype(np.int16).reshape((A, K) if lanes == 1 else (A, K, 2))


def extreme_taps(rng, A, K, lanes):
    """Every component at +-32512: 64 complex weights reach 128 sum|h| = 2^29, the bound lies beyond what the shape holds."""
    n = A * K * lanes
    h = spec.MAX_TAP * rng.choice([-1, 1], n)
    assert 128 * int(np.abs(h).sum()) < 2 ** 31
    return h.astype(np.int16).reshape((A, K) if lanes == 1 else (A, K, 2))


def same_stats(ctx, b, lanes, A, K, flags):
    want = spec.stats(b, lanes, A, K, flags)
    rec = ctx.upload(np.ascontiguousarray(b).view(np.int8))
    try:
        got = ctx.array_stats(rec, lanes, A, K, offset_binary=bool(flags))
        again = ctx.array_stats(rec, lanes, A, K, offset_binary=bool(flags))
    finally:
        rec.free()
    what = (lanes, A, K, flags, b.size)
    assert got.dtype == np.int64 and got.shape == want.shape == (A, A, K, lanes), what
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4])
    assert got.tobytes() == again.tobytes(), what                              # two calls are bit-identical
    return want


def same_combined(ctx, b, h, S, lanes, A, flags):
    want, clipped = spec.combine(b, h, S, lanes, A, flags)
    rec = ctx.upload(np.ascontiguousarray(b).view(np.int8))
    try:
        out = ctx.combine(rec, lanes, A, h, S, offset_binary=bool(flags))
        try:
            what = (lanes, A, h.shape[1], S, flags, b.size)
            assert len(out) == want.size, what
            got = out.download()
            assert got.tobytes() == want.tobytes(), \
                "%r: first difference at output byte %d" % (what, int(np.flatnonzero(got != want)[0]))
            assert out.clipped == clipped, (what, out.clipped, clipped)
        finally:
            out.free()
    finally:
        rec.free()
    return want, clipped


# ---- the statistics, exact ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("A", ANTENNAS)
def test_statistics_are_exact(ctx, pool, lanes, A):
    T = pkg()._native.array_stats_tile()
    rng = np.random.default_rng(10 * A + lanes)
    calls = 0
    for K in taps_of(A):
        for flags in (0, spec.OFFSET_BINARY):
            for F in lengths(K, T):
                start = int(rng.integers(0, 256))
                b = pool[start:start + F * A * lanes]
                assert b.size == F * A * lanes and (b.size < 2048 or np.unique(b).size == 256)
                same_stats(ctx, b, lanes, A, K, flags)
                calls += 1
    assert calls >= 3 * 2 * 8


def test_full_scale_partial_sums_are_flushed(ctx):
    """Every byte -128 at 8 antennas of I/Q: each product is 2^14, a real part takes two per frame, and more than 2^18
    frames pass 2^31 - a 32-bit partial sum that is never flushed into 64 bits shows."""
    A, K, lanes = 8, 7, 2
    F = max(3 * pkg()._native.array_stats_tile(), 2 ** 18 + 5)
    b = np.full(F * A * lanes, -128, dtype=np.int8)
    want = same_stats(ctx, b, lanes, A, K, 0)
    for d in range(K):
        assert np.all(want[:, :, d, 0] == 2 * 16384 * (F - d)) and np.all(want[:, :, d, 1] == 0)
    assert want[0, 0, 0, 0] > 2 ** 32
    # the same bytes read as offset binary are all zero
    rec = ctx.upload(np.full(64 * A * lanes, -128, dtype=np.int8))
    try:
        assert not ctx.array_stats(rec, lanes, A, K, offset_binary=True).any()
    finally:
        rec.free()


# ---- the combiner, byte for byte ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("A", ANTENNAS)
def test_combined_byte_for_byte(ctx, pool, lanes, A):
    T = pkg()._native.combine_tile() // lanes                                  # output frames of a tile
    rng = np.random.default_rng(1000 + 10 * A + lanes)
    turn = seen_clipped = seen_unclipped = 0
    for K in taps_of(A) + ("extreme",):
        for flags in (0, spec.OFFSET_BINARY):
            if K == "extreme":
                h = extreme_taps(rng, A, taps_of(A)[-1], lanes)
            for F in lengths(h.shape[1] if K == "extreme" else K, T):
                S = SHIFTS[turn % 3]
                turn += 1
                if K != "extreme":
                    h = random_taps(rng, A, K, lanes, S)
                start = int(rng.integers(0, 256))
                b = pool[start:start + F * A * lanes]
                assert b.size == F * A * lanes
                want, clipped = same_combined(ctx, b, h, S, lanes, A, flags)
                assert want.size == F * lanes
                seen_clipped += clipped > 0
                seen_unclipped += clipped < want.size
    assert turn >= 4 * 2 * 8 and seen_clipped > 10 and seen_unclipped > 10


# ---- the records' behaviour ---------------------------------------------------------------------------------------------

def other_timings(ctx):
    return (ctx.filter_timing(), ctx.iq_timing(), ctx.requant_timing(), ctx.cond_timing(), ctx.unpack_timing(),
            ctx.decim_timing(), ctx.resamp_timing())


def test_record_behaviour(ctx, pool, tmp_path):
    m = pkg()
    n = m._native
    rng = np.random.default_rng(201)
    A, K, lanes, S = 3, 5, 2, 12
    tile = n.combine_tile()
    b = pool[:A * lanes * (3 * tile // (2 * lanes) + 7)].view(np.int8)
    h = random_taps(rng, A, K, lanes, S)
    want, clipped = spec.combine(b, h, S, lanes, A)
    rho = spec.stats(b, lanes, A, K)
    assert 0 < clipped < want.size and want.size > tile + 8
    before = other_timings(ctx)
    rec = ctx.upload(b)
    try:
        got = ctx.array_stats(rec, lanes, A, K)
        t_stats = ctx.array_stats_timing()
        assert np.array_equal(got, rho) and t_stats > 0.0
        a = ctx.combine(rec, lanes, A, h, S)
        assert rec.download().tobytes() == b.tobytes()                         # the input is left alone
        ln = C.c_size_t(0)
        assert n.lib().sgx_if_length(a._h, C.byref(ln)) == n.SGX_OK and ln.value == want.size == len(a)
        assert a.download().tobytes() == want.tobytes() and a.clipped == clipped
        assert a.download(tile - 3, 11).tobytes() == want[tile - 3:tile + 8].tobytes()
        # the two timing slots are their own, every other stage's is unchanged
        assert ctx.combine_timing() > 0.0 and ctx.array_stats_timing() == t_stats and other_timings(ctx) == before
        t_comb = ctx.combine_timing()
        assert np.array_equal(ctx.array_stats(rec, lanes, A, K), rho) and ctx.combine_timing() == t_comb
        # a second call's count starts from zero, and so do its sums
        h1 = random_taps(rng, 2, 3, 1, S)
        w1, c1 = spec.combine(b, h1, S, 1, 2)
        other = ctx.combine(rec, 1, 2, h1, S)
        assert other.download().tobytes() == w1.tobytes() and other.clipped == c1
        assert np.array_equal(ctx.array_stats(rec, 1, 2, 3), spec.stats(b, 1, 2, 3))
        again = ctx.combine(rec, lanes, A, h, S)
        assert again.download().tobytes() == want.tobytes() and again.clipped == clipped
        assert np.array_equal(ctx.array_stats(rec, lanes, A, K), rho)
        # the output is an ordinary record: it goes through the stage again and is freed
        w2, c2 = spec.combine(want, h1, S, 1, 2)
        twice = ctx.combine(a, 1, 2, h1, S)
        assert twice.download().tobytes() == w2.tobytes() and twice.clipped == c2
        for r in (twice, again, other, a):
            r.free()
        assert not a._h
    finally:
        rec.free()
    # a record that is still streaming in is waited for
    path = tmp_path / "array.bin"
    long_ = np.tile(b, 6)
    long_.tofile(str(path))
    wbig, cbig = spec.combine(long_, h, S, lanes, A)
    opened = ctx.open_file(str(path), 0, long_.size)
    try:
        assert np.array_equal(ctx.array_stats(opened, lanes, A, K), spec.stats(long_, lanes, A, K))
    finally:
        opened.free()
    opened = ctx.open_file(str(path), 0, long_.size)
    try:
        out = ctx.combine(opened, lanes, A, h, S)
        assert out.download().tobytes() == wbig.tobytes() and out.clipped == cbig
        out.free()
    finally:
        opened.free()
    # the empty record: zero statistics, an empty record, zero timing slots, a zero count
    empty = ctx.upload(np.zeros(0, dtype=np.int8))
    try:
        for la in (1, 2):
            assert not ctx.array_stats(empty, la, A, K).any() and ctx.array_stats_timing() == 0.0
            out = ctx.combine(empty, la, A, h if la == 2 else h[:, :, 0], S)
            assert len(out) == 0 and out.download().size == 0 and ctx.combine_timing() == 0.0 and out.clipped == 0
            out.free()
    finally:
        empty.free()


def test_refusals_on_the_device(ctx):
    """Every refusal with a record and a context in hand; nothing is launched: the timing slots stay as they were."""
    n = pkg()._native
    good = np.arange(-6, 6, dtype=np.int16)                                    # 4 antennas x 3 taps
    rec = ctx.upload(np.zeros(4 * 250, dtype=np.int8))
    odd = ctx.upload(np.zeros(4 * 250 + 2, dtype=np.int8))
    try:
        ok = ctx.combine(rec, 1, 4, good, 12)
        ok.free()
        ctx.array_stats(rec, 1, 4, 3)
        t0 = (ctx.array_stats_timing(), ctx.combine_timing())
        assert min(t0) > 0.0
        f, g = n.lib().sgx_if_combine, n.lib().sgx_array_stats
        out, cnt = C.c_void_p(), C.c_int64(-1)
        rho = np.zeros(8 * 8 * 15 * 2, dtype=np.int64)

        def refused(word, both=True, r=rec, lanes=1, A=4, taps=good, K=3, shift=12, flags=0, c=ctx._h, o=C.byref(out)):
            rc = f(c, None if r is None else r._h, lanes, A, None if taps is None else n._ptr(taps), K, shift, flags, o,
                   C.byref(cnt))
            assert rc == n.SGX_E_ARG and word in n.last_error(), (word, rc, n.last_error())
            assert not out.value
            if both:
                rc = g(c, None if r is None else r._h, lanes, A, K, flags, n._ptr(rho))
                assert rc == n.SGX_E_ARG and word in n.last_error(), (word, rc, n.last_error())
            assert (ctx.array_stats_timing(), ctx.combine_timing()) == t0

        wide = np.zeros(8 * 17 * 2, dtype=np.int16)
        for lanes in (0, 3):
            refused("lanes", lanes=lanes, taps=wide)
        for A in (0, 1, 9):
            refused("A =", A=A, taps=wide)
        for K in (0, 2, 16, 17):
            refused("K =", K=K, taps=wide)
        refused("A K", A=8, K=9, taps=wide)
        refused("flags", flags=2)
        for S in (-1, 31):
            refused("shift", both=False, shift=S)
        refused("taps", both=False, taps=None)
        refused("taps", both=False, taps=np.full(12, 32513, dtype=np.int16))
        refused("taps", both=False, lanes=2, A=2, taps=np.tile(np.array([0, -32513], dtype=np.int16), 6))
        refused("rec", r=None)
        refused("out", both=False, o=None)
        refused("c &&", c=None)
        refused("frames", r=odd)
        refused("frames", r=rec, lanes=2, A=3, taps=np.zeros(18, dtype=np.int16))
        assert g(ctx._h, rec._h, 1, 4, 3, 0, None) == n.SGX_E_ARG and "rho" in n.last_error()
        # (128 sum|h| >= 2^31 is out of reach of 64 complex taps at full scale: 2^29)
        # no count is asked for: the call works without it
        assert f(ctx._h, rec._h, 1, 4, n._ptr(good), 3, 12, 0, C.byref(out), None) == n.SGX_OK and out.value
        assert n.lib().sgx_if_free(ctx._h, out) == n.SGX_OK
        with pytest.raises(ValueError, match="values per tap"):
            ctx.combine(rec, 2, 4, good[:11], 12)
    finally:
        odd.free()
        rec.free()


# ---- past 2^32 ----------------------------------------------------------------------------------------------------------

def test_input_beyond_two_to_the_32(ctx):
    """8 real streams in 2^32 + 196 944 bytes: the tiled record of tests/big_record.py.  The statistics at K = 1 equal the
    exact sums the record's periodicity gives; the combiner's windows (K = 3) at the start, across input bytes 2^31 and
    2^32 and at the end equal the contract's - each held to the wrap rule on the CPU first -, and so does the clip count
    of the whole."""
    n = pkg()._native
    rec = big.Tiled()
    stage = big_array.Combine(3, 12)
    A = big_array.ANTENNAS
    assert rec.n > (1 << 32) + 3 * n.combine_tile() * A and rec.n % A == 0 and (1 << 32) % rec.P and (1 << 31) % rec.P
    assert stage.width >= 2 * n.combine_tile()
    windows = stage.windows(rec)
    n_out = rec.n // A
    w = stage.width
    assert windows == [(0, w), ((1 << 31) // A - w // 2, (1 << 31) // A + w // 2),
                       ((1 << 32) // A - w // 2, (1 << 32) // A + w // 2), (n_out - w, n_out)]
    wants = [big.wrap_visible(rec.at, stage.contract(rec.n), win) for win in windows]
    head, _ = spec.combine(rec.at(0, 2 * w * A), stage.h, stage.S, 1, A)
    assert wants[0].tobytes() == head[:w].tobytes()
    clipped = stage.counters(rec)["clipped"]
    rho = big_array.stats_of(rec)
    assert rho[0, 0, 0, 0] > 2 ** 32
    b = rec.build()
    dev = ctx.upload(b)
    del b
    try:
        got = ctx.array_stats(dev, 1, A, 1)
        assert np.array_equal(got, rho), np.argwhere(got != rho)[:4]
        out = ctx.combine(dev, 1, A, stage.h, stage.S)
        try:
            assert len(out) == n_out
            for (w0, w1), want in zip(windows, wants):
                got = out.download(w0, w1 - w0)
                assert got.tobytes() == want.tobytes(), \
                    "window [%d, %d): first difference at output byte %d" % (w0, w1, w0 + int(np.flatnonzero(got != want)[0]))
            assert 0 < clipped < n_out and out.clipped == clipped
        finally:
            out.free()
    finally:
        dev.free()


# ---- end to end: the scenes ---------------------------------------------------------------------------------------------

def _same_search(a, ref):
    assert np.array_equal(a.codePhase, ref["codePhase"])
    assert np.array_equal(a.carrFreq, ref["carrFreq"])
    assert np.array_equal(np.asarray(a.internals["freqBin"]), ref["freqBin"])
    assert np.allclose(a.peakMetric, ref["peakMetric"], rtol=1e-9, atol=0)


@pytest.mark.parametrize("skip_frames", [0, cases.SKIP_FRAMES])
@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_post_processing_of_a_multi_antenna_file(tmp_path, name, skip_frames):
    m = pkg()
    scene = cases.SCENES[name]
    lanes, A = scene.lanes, cases.ANTENNAS
    b = cases.record(scene)
    path = tmp_path / ("%s.bin" % name)
    b.tofile(str(path))
    s = scene.settings(m, msToProcess=float(TRK_MS), skipNumberOfBytes=skip_frames * A * lanes)
    acq, trk, nav = s.postProcessing(str(path))
    assert nav is None or nav._solutions is None                               # 300 ms carry no subframe
    info = dict(s.lastCombining)
    fs_p, if_p = scene.prepared_rate()
    skip = skip_frames * lanes                                                 # samples of the prepared record
    assert s.antennas == A and s.skipNumberOfBytes == skip_frames * A * lanes  # left alone
    assert acq.settings.skipNumberOfBytes == skip and acq.settings.dataType == 'int8'
    assert not acq.settings.iqRecord and not acq.settings.antennas
    assert (acq.settings.samplingFreq, acq.settings.IF) == (fs_p, if_p)
    # what the run combined: the first info["samples"] / lanes frames of the file, through the contracts
    count = info["samples"]
    assert count % lanes == 0 and (skip + TRK_MS * acq.settings.samplesPerCode) < count <= b.size // A
    c = cases.combined(scene, count // lanes)
    want = c["prepared"]
    assert c["combined"].size == count == want.size
    assert (info["antennas"], info["taps"], info["reference"]) == (A, scene.K, 0)
    assert np.array_equal(info["weights"], c["weights"]) and info["suppression_db"] == c["suppression_db"]
    assert info["gain_db"] == 20.0 * float(np.log10(c["gain"])) and info["clipped"] == c["clipped"] / float(count)
    assert np.array_equal(info["input_rms"], spec.input_rms(c["rho"], count // lanes))
    with s._prepared_record(str(path), 0, want.size) as rec:
        assert rec.download().tobytes() == want.tobytes()
    assert sorted(s.lastCombining) == sorted(info) and s.lastCombining["suppression_db"] == info["suppression_db"]
    # acquisition and tracking against the oracle on that record
    n = int(acq.settings.samplesPerCode)
    o = orc.OracleSettings(samplingFreq=fs_p, IF=if_p, numberOfChannels=len(scene.prns), msToProcess=float(TRK_MS),
                           skipNumberOfBytes=skip)
    ref = orc.acquire(o, want[skip:skip + 11 * n])
    _same_search(acq, ref)
    assert sorted(np.flatnonzero(acq.carrFreq) + 1) == sorted(scene.prns)
    chans = orc.pre_run(o, ref)
    assert np.array_equal(acq.channels.PRN, chans["PRN"]) and np.count_nonzero(acq.channels.PRN) == len(scene.prns)
    series = orc.stack_series(orc.track(o, chans, want))
    same_tracking(trk, series, len(scene.prns), TRK_MS)                        # no channel lost: every block of every channel
    # the loops hold: each prompt arm carries at least half the amplitude the scene's truth predicts behind the null
    for ch in range(series.shape[0]):
        i = scene.prns.index(int(acq.channels.PRN[ch]))
        prompt = np.sqrt(np.mean(trk.series[ch, 3, 100:] ** 2))
        truth = scene.amplitude_out(i, c["weights"], c["gain"])
        print("%s PRN %d: prompt %.1f, truth %.1f" % (name, scene.prns[i], prompt, truth * n / 2.0))
        assert prompt > 0.5 * truth * n / 2.0, (ch, prompt, truth)


# ---- a packed file ------------------------------------------------------------------------------------------------------

def test_packed_four_antenna_file(tmp_path):
    """Plumbing only: a 4-bit file whose frames of four fields are four real streams goes through the unpacker, which takes
    all four, and the combiner; the prepared record is unpack_spec then array_spec byte for byte.  (No detection claim: 16
    levels limit the depth of the null.)"""
    m = pkg()
    rng = np.random.default_rng(202)
    frames, A, K = 40000, 4, 3
    common = rng.standard_normal(frames) * 5.0
    v = common[:, None] * np.array([1.0, -0.8, 0.6, 0.9])[None, :] + rng.standard_normal((frames, A)) * 1.5
    idx = np.clip(np.floor(v / 1.5 + 8.0), 0, 15).astype(np.int64)             # level 2 idx - 15
    codes = unpack_spec.code_of_level(4, unpack_spec.SIGN_MAGNITUDE)[idx].reshape(-1)
    b = unpack_spec.pack(codes, 4)
    path = tmp_path / "packed4.bin"
    b.tofile(str(path))
    s = m.Settings()
    s.samplingFreq, s.IF = 16368000.0, 4092000.0
    s.packedBits, s.packedFrame, s.antennas, s.arrayTaps, s.arrayReference = 4, 4, A, K, 2
    table = unpack_spec.table(4, unpack_spec.SIGN_MAGNITUDE, unpack_spec.DEFAULT_PEAK)
    streams = unpack_spec.unpack(b, 4, table, 0, 4, 0, 4)
    assert streams.size == frames * A
    rho = spec.stats(streams, 1, A, K)
    taps, shift, gain, supp, weights = spec.design(rho, frames, 1, 2)
    want, clipped = spec.combine(streams, taps, shift, 1, A)
    with s._prepared_record(str(path), 0, frames) as rec:
        assert rec.download().tobytes() == want.tobytes()
    assert s.lastUnpack["samples"] == frames * A
    info = s.lastCombining
    assert info["samples"] == frames and info["suppression_db"] == supp and np.array_equal(info["weights"], weights)
    assert info["clipped"] == clipped / float(frames) and supp > 3.0
    # a window from a frame on: the file range maps through both stages
    with s._prepared_record(str(path), 1000, 5000) as rec:
        part = streams[1000 * A:6000 * A]
        r2 = spec.stats(part, 1, A, K)
        t2, s2 = spec.design(r2, 5000, 1, 2)[:2]
        assert rec.download().tobytes() == spec.combine(part, t2, s2, 1, A)[0].tobytes()
