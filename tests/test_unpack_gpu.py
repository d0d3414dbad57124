"""The unpacker on the GPU (sgx_if_unpack, csrc/sgx_unpack.hip; Settings.unpackRecord, postProcessing with packedBits):
every configuration against the numpy contract of tests/unpack_spec.py byte for byte with exact code counts, the record's
behaviour, the refusals, an output beyond 2^32 bytes, then the packed files of tests/unpack_cases.py end to end against the
contracts' record and the oracle on it, by the bars of tests/test_requant_gpu.py.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import unpack_cases as cases
import unpack_spec as spec
from conftest import pkg
from oracle import softgnss_oracle as orc
from record_stage import same_tracking

pytestmark = pytest.mark.gpu

TRK_MS = 300
SCENE = cases.SCENE


@pytest.fixture(scope="module")
def ctx():
    m = pkg()
    return m.engine.get_context(m.Settings(), 0)


@pytest.fixture(scope="module")
def tile():
    return pkg()._native.unpack_tile()


def up(ctx, b):
    """The bytes b as a resident record (an empty one too)."""
    return ctx.upload(np.ascontiguousarray(b).view(np.int8))


def period(bits, frame, take):
    """(bytes, outputs) of the shortest run of whole bytes that holds whole frames."""
    w = max(1, frame * bits // 8)
    return w, w * 8 * take // (bits * frame)


def selections(frame):
    """(first, take): the first field, the last, the whole frame, its second half, two from the second on - and takes that
    are no power of two - where they fit."""
    want = [(0, 1), (frame - 1, 1), (0, frame), (frame // 2, frame // 2), (1, 2), (0, 3), (1, 5), (2, 7), (3, 13)]
    out = []
    for first, take in want:
        if take >= 1 and first + take <= frame and (first, take) not in out:
            out.append((first, take))
    return out


def random_table(rng, bits):
    """2^bits distinct int8 values, -128 and 127 among them (for 1 bit: exactly those)."""
    rest = rng.permutation(np.arange(-127, 127))[:(1 << bits) - 2]
    return rng.permutation(np.concatenate([[-128, 127], rest])).astype(np.int8)


def same(ctx, b, bits, table, flags, frame, first, take):
    """The bytes b through the library equal the contract byte for byte; so do the code counts."""
    want = spec.unpack(b, bits, table, flags, frame, first, take)
    rec = up(ctx, b)
    try:
        out = ctx.unpack(rec, bits, table, lsb_first=bool(flags & spec.LSB_FIRST), frame=frame, first=first, take=take)
        try:
            what = (bits, flags, frame, first, take, b.size)
            assert len(out) == want.size, what
            got = out.download()
            assert got.tobytes() == want.tobytes(), \
                "%r: first difference at output byte %d" % (what, int(np.flatnonzero(got != want)[0]))
            counts = spec.code_counts(b, bits, flags, frame, first, take)
            assert np.array_equal(out.code_counts, counts[:1 << bits]) and out.code_counts.dtype == np.int64, what
        finally:
            out.free()
    finally:
        rec.free()
    return want


# ---- every configuration, byte for byte --------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", spec.BITS)
def test_every_configuration_byte_for_byte(ctx, tile, bits):
    rng = np.random.default_rng(40 + bits)
    # all 256 byte values, over and over in random order: every input longer than a few hundred bytes holds them all
    pool = np.concatenate([rng.permutation(256) for _ in range(8 * (2 * tile + 5) // 256 + 2)]).astype(np.uint8)
    seen_any = seen_fast = 0
    for flags in (0, spec.LSB_FIRST):
        for frame in spec.FRAMES:
            for first, take in selections(frame):
                table = random_table(rng, bits)
                w, k = period(bits, frame, take)
                for target in (0, 1, tile - 1, tile, tile + 1, 2 * tile + 5):
                    # the whole-frame length nearest the target; "one frame" is one period
                    periods = 0 if target == 0 else max(1, int(round(target / float(k))))
                    b = pool[:periods * w]
                    assert periods * w <= pool.size and (target < tile - 1 or b.size >= 256)
                    want = same(ctx, b, bits, table, flags, frame, first, take)
                    assert want.size == periods * k
                seen_any += take & (take - 1) != 0
                seen_fast += take & (take - 1) == 0
    assert seen_any >= 8 and seen_fast >= 30                                   # both kernels were run


# ---- the record's behaviour --------------------------------------------------------------------------------------------------

def test_record_behaviour(ctx, tile, tmp_path):
    m = pkg()
    n = m._native
    case = cases.CASES["real2"]
    b = cases.file_of(case, 11)
    want = cases.unpacked(case, b)
    before = (ctx.requant_timing(), ctx.cond_timing())
    rec = up(ctx, b)
    try:
        a = ctx.unpack(rec, case.bits, case.table)
        assert rec.download().tobytes() == b.tobytes()                         # the input is left alone
        ln = C.c_size_t(0)
        assert n.lib().sgx_if_length(a._h, C.byref(ln)) == n.SGX_OK and ln.value == want.size == len(a)
        assert a.download().tobytes() == want.tobytes()
        assert a.download(tile - 3, 11).tobytes() == want[tile - 3:tile + 8].tobytes()
        assert ctx.unpack_timing() > 0.0
        assert (ctx.requant_timing(), ctx.cond_timing()) == before             # the other stages' slots are theirs
        # a second call's counts do not include the first's
        half = ctx.unpack(rec, case.bits, case.table, frame=2, first=1, take=1)
        assert np.array_equal(half.code_counts, spec.code_counts(b, 2, 0, 2, 1, 1)[:4])
        assert half.code_counts.sum() == len(half) == want.size // 2
        again = ctx.unpack(rec, case.bits, case.table)
        assert np.array_equal(again.code_counts, a.code_counts) and a.code_counts.sum() == want.size
        half.free()
        again.free()
        a.free()
    finally:
        rec.free()
    # the output is an ordinary record: searched by acquire on a context of its own settings, and freed
    real = case.settings(m)._prepared_settings()
    c2 = m.engine.get_context(real, 0)
    rec = up(c2, b)
    try:
        out = c2.unpack(rec, case.bits, case.table)
        got = c2.acquire(out, 0, 11 * SCENE.samples_per_code, np.arange(32))
        ref = cases.contract_acquisition(case)
        det = ref["carrFreq"] != 0
        assert np.array_equal(got["freqBin"][det], np.asarray(ref["freqBin"])[det])
        assert np.array_equal(got["codePhase"], ref["codePhase"])
        assert sorted(np.flatnonzero(got["carrFreq"]) + 1) == sorted(SCENE.prns)
        out.free()
        assert not out._h
    finally:
        rec.free()
    # a record that is still streaming in is waited for
    path = tmp_path / "packed.bin"
    big = np.tile(b, 8)
    big.tofile(str(path))
    opened = ctx.open_file(str(path), 0, big.size)
    try:
        out = ctx.unpack(opened, case.bits, case.table)
        assert out.download().tobytes() == np.tile(want, 8).tobytes()
        out.free()
    finally:
        opened.free()
    # the empty record: an empty record, a zero timing slot, zero counts
    empty = up(ctx, np.zeros(0, dtype=np.uint8))
    try:
        out = ctx.unpack(empty, 2, case.table, frame=4, first=1, take=2)
        assert len(out) == 0 and out.download().size == 0 and ctx.unpack_timing() == 0.0
        assert not out.code_counts.any() and out.code_counts.shape == (4,)
        out.free()
    finally:
        empty.free()


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device(ctx):
    """Every refusal once more with a record and a context in hand, the one that looks at the record among them; nothing is
    launched: the timing slot stays as it was.  (A record beyond one launch - 2^31 tiles, 2^45 samples - does not fit a
    device: that refusal is sgx_stage_one_launch's, which the stages share.)"""
    n = pkg()._native
    table = np.array([16, 48, -16, -48], dtype=np.int8)
    rec = ctx.upload(np.zeros(1001, dtype=np.int8))
    try:
        ok = ctx.unpack(rec, 2, table)
        ok.free()
        t0 = ctx.unpack_timing()
        assert t0 > 0.0

        def refused(word, **kw):
            args = dict(bits=2, table=table)
            args.update(kw)
            with pytest.raises(n.SgxError) as e:
                ctx.unpack(rec, **args)
            assert e.value.code == n.SGX_E_ARG and word in str(e.value), (kw, str(e.value))
            assert ctx.unpack_timing() == t0

        for bits in (0, 3, 8):
            refused("bits", bits=bits)
        for frame in (0, 3, 32):
            refused("frame", frame=frame)
        for first, take in ((0, 0), (-1, 1), (3, 2), (4, 1), (0, 5)):
            refused("take", frame=4, first=first, take=take)
            refused("first", frame=4, first=first, take=take)
        # fields that do not fill whole frames: 1001 bytes of 2-bit fields are no whole frames of 8 or 16 fields, 1001
        # bytes of 1-bit fields none of 16, of 4-bit fields none of 4, 8, 16
        for bits, frame in ((2, 8), (2, 16), (1, 16), (4, 4), (4, 8), (4, 16)):
            with pytest.raises(ValueError):
                spec.check(bits, 0, frame, 0, 1, 1001)
            refused("whole frames", bits=bits, frame=frame, table=np.zeros(1 << bits, dtype=np.int8))
        for bits, frame in ((2, 4), (1, 8), (4, 2), (1, 2)):
            out = ctx.unpack(rec, bits, np.zeros(1 << bits, dtype=np.int8), frame=frame)
            assert len(out) == 1001 * 8 // bits // frame
            out.free()
        t0 = ctx.unpack_timing()
        f = n.lib().sgx_if_unpack
        tab16 = np.zeros(16, dtype=np.int8)
        tp = tab16.ctypes.data_as(C.c_void_p)
        out = C.c_void_p()
        assert f(ctx._h, rec._h, 2, 2, 1, 0, 1, tp, C.byref(out), None) == n.SGX_E_ARG and "flags" in n.last_error()
        assert f(ctx._h, None, 2, 0, 1, 0, 1, tp, C.byref(out), None) == n.SGX_E_ARG and "rec" in n.last_error()
        assert f(ctx._h, rec._h, 2, 0, 1, 0, 1, None, C.byref(out), None) == n.SGX_E_ARG and "table" in n.last_error()
        assert f(ctx._h, rec._h, 2, 0, 1, 0, 1, tp, None, None) == n.SGX_E_ARG and "out" in n.last_error()
        assert f(None, rec._h, 2, 0, 1, 0, 1, tp, C.byref(out), None) == n.SGX_E_ARG
        assert not out.value and ctx.unpack_timing() == t0
        # no counts are asked for: the call works without them
        assert f(ctx._h, rec._h, 2, 0, 1, 0, 1, tp, C.byref(out), None) == n.SGX_OK and out.value
        assert n.lib().sgx_if_free(ctx._h, out) == n.SGX_OK
        with pytest.raises(ValueError, match="table"):
            ctx.unpack(rec, 2, [1, 2, 3])
    finally:
        rec.free()


# ---- past 2^32 -----------------------------------------------------------------------------------------------------------------

def test_output_beyond_two_to_the_32(ctx, tile):
    """A 1-bit input of 2^29 + T bytes: more than 4 GiB of output while the input index is still small.  Windows of 2 T
    bytes at the start, across output byte 2^32 and at the end equal the contract's; the counts are exact."""
    rng = np.random.default_rng(50)
    block = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    reps = (1 << 29) // block.size
    b = np.concatenate([np.tile(block, reps), block[:tile]])
    assert b.size == (1 << 29) + tile
    table = np.array([-37, 101], dtype=np.int8)
    n_out = 8 * b.size
    ones_of = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1)
    ones = reps * int(ones_of[block].sum()) + int(ones_of[block[:tile]].sum())
    rec = up(ctx, b)
    try:
        out = ctx.unpack(rec, 1, table, lsb_first=True)
        try:
            assert len(out) == n_out > (1 << 32)
            for start in (0, (1 << 32) - tile, n_out - 2 * tile):
                assert start % 8 == 0
                want = spec.unpack(b[start // 8:start // 8 + 2 * tile // 8], 1, table, spec.LSB_FIRST)
                got = out.download(start, 2 * tile)
                assert got.tobytes() == want.tobytes(), start
            assert list(out.code_counts) == [n_out - ones, ones] and int(out.code_counts.sum()) == n_out
        finally:
            out.free()
    finally:
        rec.free()


# ---- end to end: the four packed files -------------------------------------------------------------------------------------------

def _same_search(a, ref):
    assert np.array_equal(a.codePhase, ref["codePhase"])
    assert np.array_equal(a.carrFreq, ref["carrFreq"])
    assert np.array_equal(np.asarray(a.internals["freqBin"]), ref["freqBin"])
    assert np.allclose(a.peakMetric, ref["peakMetric"], rtol=1e-9, atol=0)


@pytest.mark.parametrize("skip", [0, cases.SKIP_SAMPLES])
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_post_processing_of_a_packed_file(tmp_path, name, skip):
    m = pkg()
    case = cases.CASES[name]
    b = cases.file_of(case, TRK_MS + 4)
    path = tmp_path / ("%s.bin" % name)
    b.tofile(str(path))
    s = case.settings(m, msToProcess=float(TRK_MS), skipNumberOfBytes=case.file_bytes(skip))
    acq, trk, nav = s.postProcessing(str(path))
    assert nav is None or nav._solutions is None                               # 300 ms carry no subframe
    info = dict(s.lastUnpack)
    count = info["samples"]                                                    # the samples that were unpacked
    assert skip + TRK_MS * SCENE.samples_per_code < count <= b.size * 8 * case.take // (case.bits * case.frame)
    assert s.packedBits == case.bits and s.iqRecord == case.iq and s.skipNumberOfBytes == case.file_bytes(skip)   # left alone
    assert acq.settings.skipNumberOfBytes == skip and acq.settings.dataType == 'int8'
    assert not acq.settings.iqRecord and not acq.settings.packedBits
    assert (acq.settings.samplingFreq, acq.settings.IF) == (SCENE.fs, SCENE.IF)
    # what the run unpacked: the table, the exact counts and shares
    head = b[:case.file_bytes(count)]
    counts = spec.code_counts(head, case.bits, case.flags, case.frame, case.first, case.take)[:1 << case.bits]
    assert info["bits"] == case.bits and np.array_equal(info["table"], case.table)
    assert np.array_equal(info["code_counts"], counts) and counts.sum() == count
    assert np.array_equal(info["shares"], counts / float(count))
    # the prepared record is the contracts', byte for byte
    want = cases.prepared(case, head)
    with s._prepared_record(str(path), 0, count) as rec:
        assert rec.download().tobytes() == want.tobytes()
    assert np.array_equal(s.lastUnpack["code_counts"], counts)
    # acquisition and tracking against the oracle on that record
    n = SCENE.samples_per_code
    o = SCENE.oracle_settings(msToProcess=float(TRK_MS), skipNumberOfBytes=skip)
    ref = orc.acquire(o, want[skip:skip + 11 * n])
    _same_search(acq, ref)
    assert sorted(np.flatnonzero(acq.carrFreq) + 1) == sorted(SCENE.prns)
    chans = orc.pre_run(o, ref)
    assert np.array_equal(acq.channels.PRN, chans["PRN"]) and np.count_nonzero(acq.channels.PRN) == len(SCENE.prns)
    same_tracking(trk, orc.stack_series(orc.track(o, chans, want)), len(SCENE.prns), TRK_MS)
