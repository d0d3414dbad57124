"""The block-adaptive antenna combiner on the GPU (sgx_array_block_stats, sgx_if_combine_blocks, csrc/sgx_array.hip;
Settings.combineAntennas with arrayBlockMs): the statistics of every block as exact int64 and the combined record byte for
byte with exact clip counts against the numpy contract of tests/array_block_spec.py - at every number of antennas the
kernels are built for, both record kinds, and the lengths at which a lag reaches across a seam, the last block is shorter
than the taps, the taps reach back into the previous block, the last tile is partial and a block holds several tiles -,
their agreement with the whole-record calls, a full-scale record whose 32-bit partial sums would wrap, the records'
behaviour and the refusals, an input beyond 2^32 bytes, and the moving-jammer scene of tests/array_block_cases.py end to end
against the contracts' record and the oracle on it.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import array_block_cases as bcases
import array_block_spec as bspec
import array_cases as cases
import array_spec as spec
import big_array
import big_record as big
from conftest import pkg
from oracle import softgnss_oracle as orc
from record_stage import same_tracking

pytestmark = pytest.mark.gpu

B = bspec.BLOCK_UNIT
ANTENNAS = (2, 3, 4, 8)
SHIFTS = (0, 12, 30)
# (block length, frames): a lag across a seam and taps that reach back over it (every F beyond B), a last block shorter than
# K (1, 4097, 8193), a partial last tile, both tiles of an I/Q unit and of the statistics (4095 .. 4097), several tiles per
# block (B = 8192)
SHAPES = [(B, F) for F in (1, 4095, 4096, 4097, 8193, 3 * 4096 - 1, 3 * 4096 + 5)] + [(2 * B, 2 * 8192 + 2049)]


def taps_of(A):
    return (1, 3, 15) if A <= 4 else (1, 3, 7)


@pytest.fixture(scope="module")
def ctx():
    m = pkg()
    return m.engine.get_context(m.Settings(), 0)


@pytest.fixture(scope="module")
def pool():
    """All 256 byte values, over and over in random order."""
    rng = np.random.default_rng(210)
    need = 16 * max(F for _, F in SHAPES) + 512
    return np.concatenate([rng.permutation(256) for _ in range(need // 256 + 2)]).astype(np.uint8)


def block_taps(rng, nb, A, K, lanes, shift):
    """Random taps inside the bound, others in every block: a wrong block index shows in the bytes."""
    h = np.stack([big.taps_in_bound(rng, A * K * lanes, shift) for _ in range(nb)]) if nb else np.zeros((0, A * K * lanes), np.int16)
    return h.reshape((nb, A, K) if lanes == 1 else (nb, A, K, 2))


# ---- the statistics, exact ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("A", ANTENNAS)
def test_block_statistics_are_exact(ctx, pool, lanes, A):
    rng = np.random.default_rng(20 * A + lanes)
    turn = 0
    for K in taps_of(A):
        for Bf, F in SHAPES:
            flags = spec.OFFSET_BINARY if turn % 2 else 0
            turn += 1
            start = int(rng.integers(0, 256))
            b = pool[start:start + F * A * lanes]
            assert b.size == F * A * lanes
            want = bspec.block_stats(b, lanes, A, K, Bf, flags)
            rec = ctx.upload(np.ascontiguousarray(b).view(np.int8))
            try:
                got = ctx.array_block_stats(rec, lanes, A, K, Bf, offset_binary=bool(flags))
                again = ctx.array_block_stats(rec, lanes, A, K, Bf, offset_binary=bool(flags))
                whole = ctx.array_stats(rec, lanes, A, K, offset_binary=bool(flags))
            finally:
                rec.free()
            what = (lanes, A, K, flags, Bf, F)
            assert got.dtype == np.int64 and got.shape == want.shape == (-(-F // Bf), A, A, K, lanes), what
            assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4])
            assert got.tobytes() == again.tobytes(), what                      # two calls are bit-identical
            assert np.array_equal(got.sum(axis=0), whole), what                # the blocks add up to the whole-record call
    assert turn == 3 * len(SHAPES)


def test_full_scale_partial_sums_are_flushed(ctx):
    """Every byte -128 at 8 antennas of I/Q over two blocks of 2^18 frames: a real part takes 2^15 per frame, so a block's
    sum passes 2^32 - a 32-bit partial sum that is not flushed per tile shows.  Block 0's lags reach into block 1."""
    A, K, lanes, Bf = 8, 7, 2, 1 << 18
    b = np.full(2 * Bf * A * lanes, -128, dtype=np.int8)
    rec = ctx.upload(b)
    try:
        got = ctx.array_block_stats(rec, lanes, A, K, Bf)
        assert got.tobytes() == ctx.array_block_stats(rec, lanes, A, K, Bf).tobytes()
        assert not ctx.array_block_stats(rec, lanes, A, K, Bf, offset_binary=True).any()
    finally:
        rec.free()
    assert got.shape == (2, A, A, K, lanes) and not got[..., 1].any()
    for d in range(K):
        assert np.all(got[0, :, :, d, 0] == 2 * 16384 * Bf) and np.all(got[1, :, :, d, 0] == 2 * 16384 * (Bf - d)), d
    assert got[0, 0, 0, 0, 0] > 2 ** 32
    assert np.array_equal(got[:, :2, :2, :3], bspec.block_stats(b.reshape(-1, A, lanes)[:, :2].reshape(-1), lanes, 2, 3, Bf))


# ---- the combiner, byte for byte ----------------------------------------------------------------------------------------

def same_combined(ctx, b, h, Bf, S, lanes, A, flags):
    want, clipped = bspec.combine_blocks(b, h, Bf, S, lanes, A, flags)
    rec = ctx.upload(np.ascontiguousarray(b).view(np.int8))
    try:
        out = ctx.combine_blocks(rec, lanes, A, h, Bf, S, offset_binary=bool(flags))
        try:
            what = (lanes, A, h.shape[2], S, flags, Bf, b.size)
            assert len(out) == want.size, what
            got = out.download()
            assert got.tobytes() == want.tobytes(), \
                "%r: first difference at output byte %d" % (what, int(np.flatnonzero(got != want)[0]))
            assert out.clipped == clipped, (what, out.clipped, clipped)
        finally:
            out.free()
        # the SAME taps in every block: the whole-record call's bytes and count
        same = np.repeat(h[:1], h.shape[0], axis=0)
        one = ctx.combine(rec, lanes, A, h[0], S, offset_binary=bool(flags))
        try:
            out = ctx.combine_blocks(rec, lanes, A, same, Bf, S, offset_binary=bool(flags))
            try:
                assert out.download().tobytes() == one.download().tobytes() and out.clipped == one.clipped, what
            finally:
                out.free()
        finally:
            one.free()
    finally:
        rec.free()
    return want, clipped


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("A", ANTENNAS)
def test_block_combined_byte_for_byte(ctx, pool, lanes, A):
    rng = np.random.default_rng(2000 + 20 * A + lanes)
    turn = seen_clipped = seen_unclipped = 0
    for K in taps_of(A):
        for Bf, F in SHAPES:
            S = SHIFTS[turn % 3]
            flags = spec.OFFSET_BINARY if (turn // 3) % 2 else 0
            turn += 1
            h = block_taps(rng, -(-F // Bf), A, K, lanes, S)
            start = int(rng.integers(0, 256))
            b = pool[start:start + F * A * lanes]
            want, clipped = same_combined(ctx, b, h, Bf, S, lanes, A, flags)
            assert want.size == F * lanes
            seen_clipped += clipped > 0
            seen_unclipped += clipped < want.size
    assert turn == 3 * len(SHAPES) and seen_clipped > 5 and seen_unclipped > 5


def test_a_seam_uses_the_output_frames_block(ctx, pool):
    """Taps that are zero but for one antenna's first or last tap, per block another antenna: the bytes next to a seam show
    which block's taps made them and that their inputs came from across the seam."""
    A, K, lanes = 3, 5, 1
    F = 3 * B
    b = pool[:F * A].view(np.int8)
    h = np.zeros((3, A, K), dtype=np.int16)
    h[0, 0, 0], h[1, 1, K - 1], h[2, 2, 0] = 1, 1, 1                           # y[f] = x_0[f + 2] | x_1[f - 2] | x_2[f + 2]
    x = b.reshape(-1, A).astype(np.int64)
    want = np.concatenate([x[2:B + 2, 0], x[B - 2:2 * B - 2, 1], x[2 * B + 2:, 2], [0, 0]])
    want = np.clip(want, -127, 127).astype(np.int8)
    assert bspec.combine_blocks(b, h, B, 0, lanes, A)[0].tobytes() == want.tobytes()
    rec = ctx.upload(b)
    try:
        out = ctx.combine_blocks(rec, lanes, A, h, B, 0)
        assert out.download().tobytes() == want.tobytes()
        out.free()
    finally:
        rec.free()


# ---- the records' behaviour ---------------------------------------------------------------------------------------------

def other_timings(ctx):
    return (ctx.filter_timing(), ctx.iq_timing(), ctx.requant_timing(), ctx.cond_timing(), ctx.unpack_timing(),
            ctx.decim_timing(), ctx.resamp_timing(), ctx.array_stats_timing(), ctx.combine_timing())


def test_record_behaviour(ctx, pool, tmp_path):
    m = pkg()
    n = m._native
    rng = np.random.default_rng(211)
    A, K, lanes, S = 3, 5, 2, 12
    F = 2 * B + 7
    b = pool[:A * lanes * F].view(np.int8)
    h = block_taps(rng, 3, A, K, lanes, S)
    want, clipped = bspec.combine_blocks(b, h, B, S, lanes, A)
    rho = bspec.block_stats(b, lanes, A, K, B)
    assert 0 < clipped < want.size
    rec = ctx.upload(b)
    try:
        ctx.array_stats(rec, lanes, A, K)
        ctx.combine(rec, lanes, A, h[0], S).free()
        before = other_timings(ctx)
        got = ctx.array_block_stats(rec, lanes, A, K, B)
        t_stats = ctx.array_block_stats_timing()
        assert np.array_equal(got, rho) and t_stats > 0.0
        a = ctx.combine_blocks(rec, lanes, A, h, B, S)
        assert rec.download().tobytes() == b.tobytes()                         # the input is left alone
        ln = C.c_size_t(0)
        assert n.lib().sgx_if_length(a._h, C.byref(ln)) == n.SGX_OK and ln.value == want.size == len(a)
        assert a.download().tobytes() == want.tobytes() and a.clipped == clipped
        assert a.download(B * lanes - 3, 11).tobytes() == want[B * lanes - 3:B * lanes + 8].tobytes()
        # the two timing slots are their own, every other stage's is unchanged
        assert ctx.combine_blocks_timing() > 0.0 and ctx.array_block_stats_timing() == t_stats and other_timings(ctx) == before
        # a second call's count starts from zero, and so do its sums; a smaller table after a larger one
        h1 = block_taps(rng, 2, 2, 3, 1, S)
        b1 = b[:2 * (B + 100)]
        w1, c1 = bspec.combine_blocks(b1, h1, B, S, 1, 2)
        small = ctx.upload(b1)
        other = ctx.combine_blocks(small, 1, 2, h1, B, S)
        assert other.download().tobytes() == w1.tobytes() and other.clipped == c1
        assert np.array_equal(ctx.array_block_stats(small, 1, 2, 3, B), bspec.block_stats(b1, 1, 2, 3, B))
        small.free()
        again = ctx.combine_blocks(rec, lanes, A, h, B, S)
        assert again.download().tobytes() == want.tobytes() and again.clipped == clipped
        assert np.array_equal(ctx.array_block_stats(rec, lanes, A, K, B), rho)
        # the whole-record calls beside them are left alone
        assert np.array_equal(ctx.array_stats(rec, lanes, A, K), rho.sum(axis=0))
        # the output is an ordinary record: it goes through a stage again and is freed
        h2 = block_taps(rng, 3, 2, 3, 1, S)
        w2, c2 = bspec.combine_blocks(want, h2, B, S, 1, 2)
        twice = ctx.combine_blocks(a, 1, 2, h2, B, S)
        assert twice.download().tobytes() == w2.tobytes() and twice.clipped == c2
        for r in (twice, again, other, a):
            r.free()
        assert not a._h
    finally:
        rec.free()
    # a record that is still streaming in is waited for
    path = tmp_path / "array_blocks.bin"
    long_ = np.tile(b, 6)
    long_.tofile(str(path))
    nb = -(-(6 * F) // B)
    hl = block_taps(rng, nb, A, K, lanes, S)
    wbig, cbig = bspec.combine_blocks(long_, hl, B, S, lanes, A)
    opened = ctx.open_file(str(path), 0, long_.size)
    try:
        assert np.array_equal(ctx.array_block_stats(opened, lanes, A, K, B), bspec.block_stats(long_, lanes, A, K, B))
    finally:
        opened.free()
    opened = ctx.open_file(str(path), 0, long_.size)
    try:
        out = ctx.combine_blocks(opened, lanes, A, hl, B, S)
        assert out.download().tobytes() == wbig.tobytes() and out.clipped == cbig
        out.free()
    finally:
        opened.free()
    # the empty record: no block, an empty record, zero timing slots, a zero count
    empty = ctx.upload(np.zeros(0, dtype=np.int8))
    try:
        for la in (1, 2):
            assert ctx.array_block_stats(empty, la, A, K, B).shape == (0, A, A, K, la) and ctx.array_block_stats_timing() == 0.0
            out = ctx.combine_blocks(empty, la, A, block_taps(rng, 0, A, K, la, S), B, S)
            assert len(out) == 0 and out.download().size == 0 and ctx.combine_blocks_timing() == 0.0 and out.clipped == 0
            out.free()
    finally:
        empty.free()


def test_refusals_on_the_device(ctx):
    """Every refusal with a record and a context in hand; nothing is launched: the timing slots stay as they were."""
    n = pkg()._native
    frames = 2 * B + 251                                                       # 3 blocks; no whole frames of 6 bytes
    good = np.tile(np.arange(-6, 6, dtype=np.int16), 3)                        # 3 blocks x 4 antennas x 3 taps
    rec = ctx.upload(np.zeros(4 * frames, dtype=np.int8))
    odd = ctx.upload(np.zeros(4 * frames + 2, dtype=np.int8))
    try:
        ctx.combine_blocks(rec, 1, 4, good.reshape(3, 4, 3), B, 12).free()
        ctx.array_block_stats(rec, 1, 4, 3, B)
        t0 = (ctx.array_block_stats_timing(), ctx.combine_blocks_timing())
        assert min(t0) > 0.0
        f, g = n.lib().sgx_if_combine_blocks, n.lib().sgx_array_block_stats
        out, cnt = C.c_void_p(), C.c_int64(-1)
        rho = np.zeros(3 * 8 * 8 * 15 * 2, dtype=np.int64)

        def refused(word, both=True, r=rec, lanes=1, A=4, taps=good, nb=3, B_=B, K=3, shift=12, flags=0, c=ctx._h,
                    o=C.byref(out)):
            rc = f(c, None if r is None else r._h, lanes, A, None if taps is None else n._ptr(taps), nb, B_, K, shift, flags, o,
                   C.byref(cnt))
            assert rc == n.SGX_E_ARG and word in n.last_error(), (word, rc, n.last_error())
            assert not out.value
            if both:
                rc = g(c, None if r is None else r._h, lanes, A, K, flags, B_, n._ptr(rho))
                assert rc == n.SGX_E_ARG and word in n.last_error(), (word, rc, n.last_error())
            assert (ctx.array_block_stats_timing(), ctx.combine_blocks_timing()) == t0

        wide = np.zeros(3 * 8 * 17 * 2, dtype=np.int16)
        for lanes in (0, 3):
            refused("lanes", lanes=lanes, taps=wide)
        for A in (0, 1, 9):
            refused("A =", A=A, taps=wide)
        for K in (0, 2, 16, 17):
            refused("K =", K=K, taps=wide)
        refused("A K", A=8, K=9, taps=wide)
        refused("flags", flags=2)
        for B_ in (0, -B, B - 16, B + 2048, 2048):                             # B off the unit
            refused("B =", B_=B_)
        for S in (-1, 31):
            refused("shift", both=False, shift=S)
        refused("taps", both=False, taps=None)
        # a tap beyond the bound in block 2 only: the text names the block
        bad = good.copy()
        bad[2 * 12 + 7] = -32513
        refused("block 2", both=False, taps=bad)
        assert "32512" in n.last_error()
        refused("rec", r=None)
        refused("out", both=False, o=None)
        refused("c &&", c=None)
        refused("frames", r=odd)
        refused("frames", r=rec, lanes=2, A=3, taps=wide)
        # sets of taps that are not one per block of the record
        for nb in (2, 4):
            refused("n_blocks", both=False, nb=nb, taps=wide)
        refused("n_blocks", both=False, B_=2 * B)
        assert g(ctx._h, rec._h, 1, 4, 3, 0, B, None) == n.SGX_E_ARG and "rho_blocks" in n.last_error()
        # no count is asked for: the call works without it
        assert f(ctx._h, rec._h, 1, 4, n._ptr(good), 3, B, 3, 12, 0, C.byref(out), None) == n.SGX_OK and out.value
        assert n.lib().sgx_if_free(ctx._h, out) == n.SGX_OK
        with pytest.raises(ValueError, match="shape"):
            ctx.combine_blocks(rec, 2, 4, good.reshape(3, 4, 3), B, 12)
    finally:
        odd.free()
        rec.free()


# ---- past 2^32 ----------------------------------------------------------------------------------------------------------

class BlockCombine(big.Stage):
    """sgx_if_combine_blocks on big_array's 8 real streams: K random taps per antenna and block, the table repeating every
    105 blocks - 105 x 4096 frames are four periods of the tiled record.  A chunk starts on a block."""
    name = "combine_blocks"
    num, den, unit = 1, big_array.ANTENNAS, big_array.ANTENNAS * B
    PERIOD = 105

    def __init__(self, K=3, S=12, seed=19):
        rng = np.random.default_rng(seed)
        A = big_array.ANTENNAS
        self.table = np.stack([big.taps_in_bound(rng, A * K, S) for _ in range(self.PERIOD)]).reshape(self.PERIOD, A, K)
        self.S, self.halo = S, A * ((K - 1) // 2 + 1)

    def taps(self, j0, nb):
        return self.table[(j0 + np.arange(nb)) % self.PERIOD]

    def run(self, chunk, lo):
        A = big_array.ANTENNAS
        assert lo % self.unit == 0
        nb = -(-(chunk.size // A) // B)
        y, clipped = bspec.combine_blocks(chunk, self.taps(lo // self.unit, nb), B, self.S, 1, A)
        return y, dict(clipped=clipped)

    def clipped_of(self, rec):
        """The clip count of the whole tiled record: outputs repeat with PERIOD blocks = 4 periods of the record, so with
        f(k) the contract's count on k such stretches and the rest, the record's is f(2) + (reps - 2) (f(3) - f(2))."""
        stretch = 4 * rec.P
        assert stretch == self.PERIOD * self.unit
        reps, rest = divmod(rec.n, stretch)
        assert reps >= 3

        def f(k):
            return self.run(np.concatenate([rec.at(0, stretch)] * k + [rec.at(0, rest)]), 0)[1]["clipped"]

        f2, f3 = f(2), f(3)
        return f2 + (reps - 2) * (f3 - f2)


def test_input_beyond_two_to_the_32(ctx):
    """8 real streams in 2^32 + 196 944 bytes, 131 078 blocks of 4096 frames and one of 42: the combiner's windows (K = 3, taps that
    depend on the block and repeat every 105) at the start, across input bytes 2^31 and 2^32 and at the end equal the
    contract's - each held to the wrap rule on the CPU first -, and so does the clip count of the whole; the block
    statistics at K = 1 equal the contract's, where the record's period makes block j + 105 equal block j."""
    n = pkg()._native
    rec = big.Tiled()
    stage = BlockCombine(3, 12)
    A = big_array.ANTENNAS
    frames = rec.n // A
    nb = -(-frames // B)
    assert rec.n == (1 << 32) + 196944 and rec.n % A == 0 and nb == 131079 and stage.width >= 2 * n.combine_tile()
    windows = stage.windows(rec)
    n_out = rec.n // A
    w = stage.width
    assert windows == [(0, w), ((1 << 31) // A - w // 2, (1 << 31) // A + w // 2),
                       ((1 << 32) // A - w // 2, (1 << 32) // A + w // 2), (n_out - w, n_out)]
    wants = [big.wrap_visible(rec.at, stage.contract(rec.n), win) for win in windows]
    # (a window holds the seams of four blocks or more, each with taps of its own)
    assert all(len(set(range(w0 // B, (w1 - 1) // B + 1))) >= 4 for w0, w1 in windows)
    clipped = stage.clipped_of(rec)
    # the statistics: the first 105 blocks over and over, and the short last block
    period = bspec.block_stats(rec.at(0, stage.PERIOD * B * A), 1, A, 1, B)
    assert period.shape[0] == stage.PERIOD and frames % B == 42
    last = bspec.block_stats(rec.at((nb - 1) * B * A, rec.n), 1, A, 1, B)
    assert np.array_equal(period.sum(axis=0) * ((nb - 1) // stage.PERIOD) + period[:(nb - 1) % stage.PERIOD].sum(axis=0) + last[0],
                          big_array.stats_of(rec))
    taps = stage.taps(0, nb)
    b = rec.build()
    dev = ctx.upload(b)
    del b
    try:
        got = ctx.array_block_stats(dev, 1, A, 1, B)
        assert got.shape == (nb, A, A, 1, 1)
        idx = np.arange(nb - 1) % stage.PERIOD
        diff = np.flatnonzero(np.any(got[:nb - 1].reshape(nb - 1, -1) != period.reshape(stage.PERIOD, -1)[idx], axis=1))
        assert diff.size == 0, diff[:4]
        assert np.array_equal(got[nb - 1], last[0])
        out = ctx.combine_blocks(dev, 1, A, taps, B, stage.S)
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


# ---- end to end: the moving-jammer scene --------------------------------------------------------------------------------

def _same_search(a, ref):
    assert np.array_equal(a.codePhase, ref["codePhase"])
    assert np.array_equal(a.carrFreq, ref["carrFreq"])
    assert np.array_equal(np.asarray(a.internals["freqBin"]), ref["freqBin"])
    assert np.allclose(a.peakMetric, ref["peakMetric"], rtol=1e-9, atol=0)


@pytest.fixture(scope="module")
def scene_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("moving") / "moving.bin"
    bcases.record().tofile(str(path))
    return str(path)


@pytest.mark.parametrize("skip_frames", [0, bcases.SKIP_FRAMES])
def test_post_processing_of_the_moving_jammer_file(scene_file, skip_frames):
    m = pkg()
    scene = bcases.SCENE
    lanes, A, Bf, TRK_MS = scene.lanes, bcases.ANTENNAS, bcases.BLOCK_FRAMES, bcases.TRK_MS
    b = bcases.record()
    s = scene.settings(m, msToProcess=float(TRK_MS), skipNumberOfBytes=skip_frames * A * lanes, arrayBlockMs=bcases.BLOCK_MS)
    acq, trk, nav = s.postProcessing(scene_file)
    assert nav is None or nav._solutions is None                               # 100 ms carry no subframe
    info = dict(s.lastCombining)
    fs_p, if_p = scene.prepared_rate()
    skip = skip_frames * lanes                                                 # samples of the prepared record
    assert s.antennas == A and s.skipNumberOfBytes == skip_frames * A * lanes and s.arrayBlockMs == bcases.BLOCK_MS
    assert acq.settings.skipNumberOfBytes == skip and not acq.settings.iqRecord and not acq.settings.antennas
    assert (acq.settings.samplingFreq, acq.settings.IF) == (fs_p, if_p)
    # what the run combined: the first info["samples"] / lanes frames of the file, blocks counted from its first frame
    count = info["samples"]
    assert count % lanes == 0 and (skip + TRK_MS * acq.settings.samplesPerCode) < count <= b.size // A
    frames = count // lanes
    c = bcases.combined_blocks(scene, frames)
    want = c["prepared"]
    nb = -(-frames // Bf)
    assert c["combined"].size == count == want.size and not c["status"].any()
    assert (info["antennas"], info["taps"], info["reference"]) == (A, scene.K, 0)
    assert (info["block_frames"], info["blocks"], info["window_blocks"], info["held_blocks"]) == (Bf, nb, bcases.WINDOW, 0)
    assert info["weights"].shape == (nb, A, scene.K) and np.array_equal(info["weights"], c["weights"])
    assert np.array_equal(info["block_suppression_db"], c["suppression_db"])
    assert np.array_equal(info["block_gain_db"], 20.0 * np.log10(c["gain"]))
    assert info["suppression_db"] == float(np.median(c["suppression_db"])) and info["suppression_db_min"] == c["suppression_db"].min()
    assert info["gain_db"] == float(np.median(20.0 * np.log10(c["gain"]))) and info["clipped"] == c["clipped"] / float(count)
    assert np.array_equal(info["input_rms"], spec.input_rms(c["rho"].sum(axis=0), frames))
    assert info["suppression_db_min"] > 16.0
    with s._prepared_record(scene_file, 0, want.size) as rec:
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
    same_tracking(trk, series, len(scene.prns), TRK_MS)


def test_the_composed_contract_and_the_switch(scene_file):
    """A window of the prepared record from a frame on: blocks count from the first frame handed to the stage.  The same
    file with arrayBlockMs = 0 takes the whole-record path and gives the bytes array_spec predicts."""
    m = pkg()
    scene = bcases.SCENE
    lanes = scene.lanes
    first, frames = 1000, 3 * bcases.BLOCK_FRAMES + 77
    s = scene.settings(m, arrayBlockMs=bcases.BLOCK_MS)
    c = bcases.combined_blocks(scene, frames, first)
    with s._prepared_record(scene_file, first * lanes, frames * lanes) as rec:
        assert rec.download().tobytes() == c["prepared"].tobytes()
    assert s.lastCombining["blocks"] == 4 and np.array_equal(s.lastCombining["weights"], c["weights"])
    # a window of five, blocks of two units
    s.arrayBlockMs, s.arrayWindowBlocks = 2.0, 5
    frames = 6 * bcases.BLOCK_FRAMES
    c = bcases.combined_blocks(scene, frames, 0, B=2 * bcases.BLOCK_FRAMES, W=5)
    with s._prepared_record(scene_file, 0, frames * lanes) as rec:
        assert rec.download().tobytes() == c["prepared"].tobytes()
    assert (s.lastCombining["blocks"], s.lastCombining["block_frames"], s.lastCombining["window_blocks"]) == (3, 8192, 5)
    # the switch off: today's path, today's keys
    s.arrayBlockMs = 0
    frames = cases.ACQ_MS * scene.frames_per_ms
    w = bcases.combined_whole(scene, frames)
    with s._prepared_record(scene_file, 0, frames * lanes) as rec:
        assert rec.download().tobytes() == w["prepared"].tobytes()
    info = s.lastCombining
    assert sorted(info) == ["antennas", "clipped", "gain_db", "input_rms", "reference", "samples", "suppression_db", "taps", "weights"]
    assert info["suppression_db"] == w["suppression_db"] and np.array_equal(info["weights"], w["weights"])
