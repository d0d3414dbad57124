"""The decimation stage on the GPU (sgx_if_decimate, csrc/sgx_decim.hip; Settings.decimateRecord, postProcessing with
decimation): every factor, both record kinds and the lengths at which plane seams, zero padding, the last partial store
and the tile seams lie against the numpy contract of tests/decim_spec.py byte for byte with exact clip counts, the
record's behaviour, the refusals, an input beyond 2^32 bytes whose period hides no wrapped address, then the scenes of
tests/decim_cases.py end to end against the contracts' record and the oracle on it.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import big_record as big
import decim_cases as cases
import decim_spec as spec
from conftest import pkg
from oracle import softgnss_oracle as orc
from record_stage import same_tracking

pytestmark = pytest.mark.gpu

TRK_MS = cases.TRK_MS
SHIFTS = (0, 14, 30)


@pytest.fixture(scope="module")
def ctx():
    m = pkg()
    return m.engine.get_context(m.Settings(), 0)


@pytest.fixture(scope="module")
def tile():
    return pkg()._native.decim_tile()


@pytest.fixture(scope="module")
def pool(tile):
    """All 256 byte values, over and over in random order: every input longer than a few hundred bytes holds them all."""
    rng = np.random.default_rng(160)
    need = 2 * (2 * tile * spec.MAX_FACTOR + 5 * spec.MAX_FACTOR)
    return np.concatenate([rng.permutation(256) for _ in range(need // 256 + 2)]).astype(np.uint8)


def random_taps(rng, n, shift):
    """n tap components whose sums land on both sides of the clip at this shift, inside the bound on sum|h|."""
    budget = (2 ** 31 - 1) // 128
    a = 100.0 * 2.0 ** shift * np.sqrt(3.0) / (74.0 * np.sqrt(n))
    a = int(min(max(a, 1.0), spec.MAX_TAP, 1.6 * budget / n))                  # (sum|h| is about n a / 2)
    h = rng.integers(-a, a + 1, n)
    assert 128 * int(np.abs(h).sum()) < 2 ** 31
    return h.astype(np.int16)


def extreme_taps(rng, n):
    """Components at +-32512, as many as the bound 128 sum|h| < 2^31 admits, and the rest of the bound in one more."""
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


def same(ctx, b, h, S, lanes, D, flags):
    """The bytes b through the library equal the contract byte for byte; so does the clip count."""
    want, clipped = spec.decimate(b, h, S, lanes, D, flags)
    rec = ctx.upload(np.ascontiguousarray(b).view(np.int8))
    try:
        out = ctx.decimate(rec, lanes, h, S, D, offset_binary=bool(flags & spec.OFFSET_BINARY))
        try:
            what = (lanes, D, h.size // lanes, S, flags, b.size)
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


# ---- every factor, byte for byte ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", range(spec.MIN_FACTOR, spec.MAX_FACTOR + 1))
@pytest.mark.parametrize("lanes", [1, 2])
def test_every_factor_byte_for_byte(ctx, tile, pool, lanes, D):
    rng = np.random.default_rng(1000 * lanes + D)
    T = tile // lanes                                                          # output frames of a tile
    lengths = sorted(set([1, 3, 2 * D - 1, 2 * D + 1, 63, 511]))
    turn = 0
    seen_clipped = seen_unclipped = 0
    for L in lengths + ["extreme"]:
        for flags in (0, spec.OFFSET_BINARY):
            if L == "extreme":
                h = extreme_taps(rng, lanes * 511)
            frames = sorted(set([0, 1, D - 1, D, D + 1, h.size // lanes - 1 if L == "extreme" else L - 1,
                                 511 if L == "extreme" else L, T * D - 1, T * D, T * D + 1, 2 * T * D + 5]))
            for F in frames:
                S = SHIFTS[turn % 3]
                turn += 1
                if L != "extreme":
                    h = random_taps(rng, lanes * L, S)
                start = int(rng.integers(0, 256))
                b = pool[start:start + F * lanes]
                assert b.size == F * lanes and (b.size < 1024 or np.unique(b).size == 256)
                want, clipped = same(ctx, b, h, S, lanes, D, flags)
                assert want.size == -(-F // D) * lanes
                seen_clipped += clipped > 0
                seen_unclipped += clipped < want.size
    assert turn >= 3 * len(lengths) and seen_clipped > 10 and seen_unclipped > 10


# ---- the record's behaviour ---------------------------------------------------------------------------------------------

def test_record_behaviour(ctx, tile, pool, tmp_path):
    m = pkg()
    n = m._native
    rng = np.random.default_rng(161)
    D, L = 5, 63
    b = pool[:2 * (3 * tile * D // 2 + 7)].view(np.int8)
    h = random_taps(rng, 2 * L, 14)
    want, clipped = spec.decimate(b, h, 14, 2, D)
    assert 0 < clipped < want.size
    before = (ctx.filter_timing(), ctx.iq_timing(), ctx.requant_timing(), ctx.cond_timing(), ctx.unpack_timing())
    rec = ctx.upload(b)
    try:
        a = ctx.decimate(rec, 2, h, 14, D)
        assert rec.download().tobytes() == b.tobytes()                         # the input is left alone
        ln = C.c_size_t(0)
        assert n.lib().sgx_if_length(a._h, C.byref(ln)) == n.SGX_OK and ln.value == want.size == len(a)
        assert a.download().tobytes() == want.tobytes() and a.clipped == clipped
        assert a.download(tile - 3, 11).tobytes() == want[tile - 3:tile + 8].tobytes()
        assert ctx.decim_timing() > 0.0
        # the other seven timing slots are their stages'
        assert (ctx.filter_timing(), ctx.iq_timing(), ctx.requant_timing(), ctx.cond_timing(), ctx.unpack_timing()) == before
        # a second call's count starts from zero
        h1 = random_taps(rng, L, 14)
        w1, c1 = spec.decimate(b, h1, 14, 1, 3)
        other = ctx.decimate(rec, 1, h1, 14, 3)
        assert other.download().tobytes() == w1.tobytes() and other.clipped == c1
        again = ctx.decimate(rec, 2, h, 14, D)
        assert again.download().tobytes() == want.tobytes() and again.clipped == clipped
        # the output is an ordinary record: it goes through the stage again and is freed
        twice = ctx.decimate(a, 1, h1, 14, 2)
        w2, c2 = spec.decimate(want, h1, 14, 1, 2)
        assert twice.download().tobytes() == w2.tobytes() and twice.clipped == c2
        for r in (twice, again, other, a):
            r.free()
        assert not a._h
    finally:
        rec.free()
    # a record that is still streaming in is waited for
    path = tmp_path / "decim.bin"
    big = np.tile(b, 6)
    big.tofile(str(path))
    wbig, cbig = spec.decimate(big, h, 14, 2, D)
    opened = ctx.open_file(str(path), 0, big.size)
    try:
        out = ctx.decimate(opened, 2, h, 14, D)
        assert out.download().tobytes() == wbig.tobytes() and out.clipped == cbig
        out.free()
    finally:
        opened.free()
    # the empty record: an empty record, a zero timing slot, a zero count
    empty = ctx.upload(np.zeros(0, dtype=np.int8))
    try:
        for lanes in (1, 2):
            out = ctx.decimate(empty, lanes, h[:lanes * 3], 14, D)
            assert len(out) == 0 and out.download().size == 0 and ctx.decim_timing() == 0.0 and out.clipped == 0
            out.free()
    finally:
        empty.free()


def test_the_output_is_searched_by_acquire():
    """The decimated record of scene b at D = 5 under a context of its own settings: sgx_acquire finds what the oracle
    finds on the contract's record."""
    m = pkg()
    case = cases.CASES["real_d5"]
    b = cases.file_of(case, cases.ACQ_MS)
    want = cases.prepared(case, cases.ACQ_MS)
    real = case.settings(m)._prepared_settings()
    c2 = m.engine.get_context(real, 0)
    rec = c2.upload(b)
    try:
        out = c2.decimate(rec, 1, case.taps, case.shift, case.D)
        assert out.download().tobytes() == want.tobytes()
        n = real.samplesPerCode
        got = c2.acquire(out, 0, 11 * n, np.arange(32))
        ref = cases.contract_acquisition(case)
        det = np.asarray(ref["carrFreq"]) != 0
        assert np.array_equal(got["freqBin"][det], np.asarray(ref["freqBin"])[det])
        assert np.array_equal(got["codePhase"], ref["codePhase"])
        assert sorted(np.flatnonzero(got["carrFreq"]) + 1) == sorted(case.scene.prns)
        out.free()
    finally:
        rec.free()


def test_uint8_q_first_file_prepares_the_same_record(tmp_path):
    """Scene a's file as an RTL-SDR with swapped channels would have written it - offset binary, Q before I - through
    Settings: the stage's offset-binary flag and conjugated taps, then the converter told int8 and Q first, make the record
    the plain file makes, which is the contracts'."""
    m = pkg()
    case = cases.CASES["iq_d4_63"]
    b = cases.file_of(case, cases.ACQ_MS)
    want = cases.prepared(case, cases.ACQ_MS)
    plain, swapped = tmp_path / "iq.bin", tmp_path / "qi_u8.bin"
    b.tofile(str(plain))
    (b.view(np.uint8) ^ 0x80).reshape(-1, 2)[:, ::-1].ravel().tofile(str(swapped))
    for path, kw in ((plain, {}), (swapped, dict(dataType='uint8', iqQFirst=True))):
        s = case.settings(m, **kw)
        with s._prepared_record(str(path), 0, want.size) as rec:
            assert rec.download().tobytes() == want.tobytes(), kw
        assert s.lastDecimation["samples"] == want.size and s.lastDecimation["clipped"] == 0.0


# ---- refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device(ctx):
    """Every refusal once more with a record and a context in hand, the one that looks at the record among them; nothing is
    launched: the timing slot stays as it was."""
    n = pkg()._native
    good = np.arange(-31, 32, dtype=np.int16)
    rec = ctx.upload(np.zeros(1000, dtype=np.int8))
    odd = ctx.upload(np.zeros(1001, dtype=np.int8))
    try:
        ok = ctx.decimate(rec, 1, good, 14, 4)
        ok.free()
        t0 = ctx.decim_timing()
        assert t0 > 0.0
        f = n.lib().sgx_if_decimate
        out, cnt = C.c_void_p(), C.c_int64(-1)

        def refused(word, r=rec, lanes=1, taps=good, n_taps=63, shift=14, D=4, flags=0, c=ctx._h, o=C.byref(out)):
            rc = f(c, None if r is None else r._h, lanes, None if taps is None else n._ptr(taps), n_taps, shift, D, flags, o,
                   C.byref(cnt))
            assert rc == n.SGX_E_ARG and word in n.last_error(), (word, rc, n.last_error())
            assert not out.value and ctx.decim_timing() == t0

        for lanes in (0, 3):
            refused("lanes", lanes=lanes)
        for D in (0, 1, 17):
            refused("D", D=D)
        for L in (0, 2, 62, 513):
            refused("n_taps", taps=np.zeros(1026, dtype=np.int16), n_taps=L)
        for S in (-1, 31):
            refused("shift", shift=S)
        refused("flags", flags=2)
        refused("taps", taps=None)
        refused("taps", taps=np.full(63, 32513, dtype=np.int16))
        refused("taps", lanes=2, taps=np.tile(np.array([0, -32513], dtype=np.int16), 31), n_taps=31)
        # (128 sum|h| >= 2^31 is out of reach of 511 real taps; 259 complex ones at full scale pass it)
        refused("sum", lanes=2, taps=np.full(2 * 259, 32512, dtype=np.int16), n_taps=259)
        refused("rec", r=None)
        refused("out", o=None)
        refused("c &&", c=None)
        refused("pairs", r=odd, lanes=2, taps=np.zeros(126, dtype=np.int16))
        # lanes 1 takes the odd record; no count is asked for: the call works without it
        assert f(ctx._h, odd._h, 1, n._ptr(good), 63, 14, 4, 0, C.byref(out), None) == n.SGX_OK and out.value
        assert n.lib().sgx_if_free(ctx._h, out) == n.SGX_OK
        with pytest.raises(ValueError, match="pairs"):
            ctx.decimate(rec, 2, good, 14, 4)
    finally:
        odd.free()
        rec.free()


# ---- past 2^32 ----------------------------------------------------------------------------------------------------------

def test_input_beyond_two_to_the_32(ctx, tile):
    """A real input of 2^32 + 196 944 bytes at D = 16, L = 31: the tiled record of tests/big_record.py, a random block of
    105 * 2^13 bytes over and over.  That length divides neither 2^31 nor 2^32, so byte p and byte p - 2^32 differ and a load
    address cut to 32 bits shows (a block of 2^20 bytes would hide it: tests/test_big_record_host.py).  Windows at
    the start, across input bytes 2^31 and 2^32 and at the end equal the contract's - each held to the wrap rule on the CPU
    first -, and so does the clip count of the whole."""
    D, L, S = 16, 31, 14
    rec = big.Tiled()
    stage = big.Decim(D, L, S)
    assert rec.n > (1 << 32) + 3 * tile * D and stage.width >= 2 * tile and (1 << 32) % rec.P and (1 << 31) % rec.P
    windows = stage.windows(rec)
    n_out = -(-rec.n // D)
    w = stage.width
    assert windows == [(0, w), ((1 << 31) // D - w // 2, (1 << 31) // D + w // 2),
                       ((1 << 32) // D - w // 2, (1 << 32) // D + w // 2), (n_out - w, n_out)]
    wants = [big.wrap_visible(rec.at, stage.contract(rec.n), win) for win in windows]
    # the contract itself on the head and on the tail of the record, zeros in front and behind
    head, _ = spec.decimate(rec.at(0, 2 * w * D), stage.h, S, 1, D)
    assert wants[0].tobytes() == head[:w].tobytes()
    clipped = stage.counters(rec)["clipped"]
    b = rec.build()
    dev = ctx.upload(b)
    del b
    try:
        out = ctx.decimate(dev, 1, stage.h, S, D)
        try:
            assert len(out) == n_out == rec.n // D
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


@pytest.mark.parametrize("skip_groups", [0, cases.SKIP_GROUPS])
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_post_processing_of_a_decimated_file(tmp_path, name, skip_groups):
    m = pkg()
    case = cases.CASES[name]
    scene = case.scene
    ms = TRK_MS + 4
    b = cases.file_of(case, ms)
    path = tmp_path / ("%s.bin" % name)
    b.tofile(str(path))
    skip_frames = case.D * skip_groups                                         # input frames; a multiple of D
    s = case.settings(m, msToProcess=float(TRK_MS), skipNumberOfBytes=skip_frames * case.lanes)
    acq, trk, nav = s.postProcessing(str(path))
    assert nav is None or nav._solutions is None                               # 1 s carries no subframe
    info = dict(s.lastDecimation)
    fs_p, if_p = case.prepared_rate()
    skip = skip_groups * case.lanes                                            # samples of the prepared record
    assert s.decimation == case.D and s.skipNumberOfBytes == skip_frames * case.lanes       # left alone
    assert acq.settings.skipNumberOfBytes == skip and acq.settings.dataType == 'int8'
    assert not acq.settings.iqRecord and not acq.settings.decimation
    assert (acq.settings.samplingFreq, acq.settings.IF) == (fs_p, if_p)
    # what the run decimated: the first info["samples"] bytes of the contract's record, with the contract's clip count
    count = info["samples"]
    assert count % case.lanes == 0 and (skip + TRK_MS * acq.settings.samplesPerCode) < count <= b.size // case.D
    want_dec, clipped, want = cases.prepared_head(case, ms, count // case.lanes)
    assert want_dec.size == count == want.size
    assert info["factor"] == case.D and info["taps"] == case.L and info["clipped"] == clipped / float(count)
    assert (info["fs_out"], info["f_out"], info["inverted"]) == case.design_out
    with s._prepared_record(str(path), 0, want.size) as rec:
        assert rec.download().tobytes() == want.tobytes()
    assert s.lastDecimation == info
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
    # the loops hold: the prompt arm carries the signal, at the amplitude the scene gave it (the bar of test_iq_gpu.py)
    for ch in range(series.shape[0]):
        i = scene.prns.index(int(acq.channels.PRN[ch]))
        prompt = np.sqrt(np.mean(trk.series[ch, 3, 100:] ** 2))
        assert prompt > 0.5 * case.amplitude_out(i) * n / 2.0, (ch, prompt)
