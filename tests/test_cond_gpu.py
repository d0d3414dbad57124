"""The front-end conditioning stage on the GPU (sgx_cond_block_stats, sgx_if_condition, csrc/sgx_cond.hip;
Settings.conditionRecord, postProcessing with frontEndConditioning): the statistics against the numpy contract of
tests/cond_spec.py field for field, the conditioned record byte for byte with both counters, then the capture of
tests/cond_cases.py end to end against the contracts' record and the oracle on it, by the bars of tests/test_iq_gpu.py, and
a real int16 record tracked by trk3_kernel after conditioning.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import cond_cases as cases
import cond_spec as spec
from conftest import pkg
from oracle import softgnss_oracle as orc
from record_stage import same_tracking

pytestmark = pytest.mark.gpu

TRK_MS = 300
SCENE = cases.SCENE
FORMATS = [(L, dt) for L in (1, 2) for dt in ("int8", "uint8", "int16")]
BLOCKS = (256, 272, 16384)


@pytest.fixture(scope="module")
def ctx():
    m = pkg()
    return m.engine.get_context(m.Settings(), 0)


@pytest.fixture(scope="module")
def tile():
    return pkg()._native.cond_tile()


def up(ctx, x):
    """The bytes of x as a resident record (an empty one too)."""
    return ctx.upload(np.frombuffer(np.ascontiguousarray(x).tobytes(), dtype=np.int8))


def frame_counts(B, tile=None):
    f = [0, 1, 2, 15, 16, 17, B - 1, B, B + 1, 3 * B + 5]
    if tile:
        f += [tile - 1, tile, tile + 1, 3 * tile + 5]
    return f


def extremes(dtype):
    info = np.iinfo(np.dtype(dtype))
    return int(info.min), int(info.max)


def random_record(rng, dtype, n):
    lo, hi = extremes(dtype)
    return rng.integers(lo, hi + 1, n).astype(np.dtype(dtype).newbyteorder("<"))


# ---- statistics --------------------------------------------------------------------------------------------------------------

def same_stats(ctx, x, dtype, L, B, q4):
    want = spec.block_stats(x, dtype, L, B, q4)
    rec = up(ctx, x)
    try:
        got = ctx.cond_stats(rec, dtype, L, B, q4)
    finally:
        rec.free()
    assert got.dtype == spec.STATS_DTYPE and got.shape == want.shape, (dtype, L, B, q4, x.size, got.shape, want.shape)
    for k in spec.STATS_DTYPE.names:
        assert np.array_equal(got[k], want[k]), (dtype, L, B, q4, x.size // L, k, got[k][:4], want[k][:4])
    return want


@pytest.mark.parametrize("L,dtype", FORMATS)
def test_statistics_equal_the_contract(ctx, L, dtype):
    rng = np.random.default_rng(40 + L)
    lo, hi = extremes(dtype)
    dt = np.dtype(dtype).newbyteorder("<")
    qs = (0, 16, 256, 4096)
    for B in BLOCKS:
        for i, F in enumerate(frame_counts(B)):
            n = F * L
            same_stats(ctx, random_record(rng, dtype, n), dtype, L, B, qs[i % 4])
            st = same_stats(ctx, np.full(n, 37, dtype=dt), dtype, L, B, 256)                 # all-constant: P = 0
            assert not st["p_all"].any() and np.array_equal(st["kept"], st["n"])
            same_stats(ctx, np.full(n, lo, dtype=dt), dtype, L, B, 16)                       # the most negative sums
            alt = np.full(n, lo, dtype=dt)
            alt[1::2] = hi
            same_stats(ctx, alt, dtype, L, B, 4096)                                          # alternating extremes
            alt = np.full((F, L), lo, dtype=dt)
            alt[1::2] = hi
            same_stats(ctx, alt, dtype, L, B, qs[(i + 1) % 4])                               # ... frame by frame
            if F < 17:
                continue
            # one outlier frame per block: the first, the last, a middle frame
            base = rng.integers(-20, 21, (F, L)).astype(dt) if dtype != "uint8" else rng.integers(108, 149, (F, L)).astype(dt)
            K = -(-F // B)
            for where in ("first", "last", "middle"):
                x = base.copy()
                for k in range(K):
                    nk = min(F, (k + 1) * B) - k * B
                    x[k * B + {"first": 0, "last": nk - 1, "middle": nk // 2}[where]] = hi
                for q4 in qs:
                    st = same_stats(ctx, x, dtype, L, B, q4)
                    full = st["n"] >= 256
                    if q4 in (0, 256):                           # c = 4 drops the outlier alone; no blanking keeps all
                        assert np.all(st["kept"][full] == st["n"][full] - (1 if q4 else 0)), (where, q4, st[:2])


def test_statistics_of_a_streaming_record_and_timing(ctx, tmp_path):
    x = random_record(np.random.default_rng(41), "int16", 2 * (3 * 4096 + 5))
    want = spec.block_stats(x, "int16", 2, 272, 256)
    path = tmp_path / "wide.bin"
    x.tofile(str(path))
    opened = ctx.open_file(str(path), 0, x.nbytes)                                # still streaming in when the call is made
    try:
        got = ctx.cond_stats(opened, "int16", 2, 272, 256)
        assert got.tobytes() == want.tobytes()
        assert ctx.cond_timing()[0] > 0.0
        assert ctx.cond_stats(opened, "int16", 2, 272, 256).tobytes() == want.tobytes()
    finally:
        opened.free()


# ---- apply -------------------------------------------------------------------------------------------------------------------

def varied_plan(K, theta):
    """Neighbouring entries differ in all five fields."""
    p = np.zeros(K, dtype=spec.PLAN_DTYPE)
    k = np.arange(K)
    p["dc0"], p["dc1"] = 40 * (k % 5) - 77, 63 - 31 * (k % 4)
    p["mult"], p["shift"] = 9000 + 3571 * (k % 6), 3 + (k % 3)
    p["theta"] = theta + 1009 * (k % 7)
    return p


def same_apply(ctx, x, dtype, L, B, plan, G):
    want, blanked, clipped = spec.condition(x, dtype, L, B, plan, G)
    rec = up(ctx, x)
    try:
        out = ctx.condition(rec, dtype, L, B, plan, G)
        try:
            assert len(out) == want.size
            got = out.download()
            assert got.tobytes() == want.tobytes(), "%s, L = %d, B = %d, F = %d, G = %d: first difference at element %d" % (
                dtype, L, B, want.size // L, G, int(np.flatnonzero(got != want)[0]))
            assert (out.blanked, out.clipped) == (blanked, clipped), (dtype, L, B, want.size // L, G)
        finally:
            out.free()
    finally:
        rec.free()
    return want, blanked, clipped


def hit_places(F, B, tile, G):
    """Frames 0 and F - 1, both sides of a block boundary and of a tile seam, two hits 2 G + 1 and two 2 G + 2 apart."""
    at = [0, F - 1, B - 1, B, 2 * B - 1, tile - 1, tile, 2 * tile, 2 * tile - 1]
    for start, gap in ((B + 200, 2 * G + 1), (B + 600, 2 * G + 2), (tile - G - 1, 2 * G + 1), (2 * tile - G - 1, 2 * G + 2)):
        at += [start, start + gap]
    return sorted(set(f for f in at if 0 <= f < F))


@pytest.mark.parametrize("L,dtype", FORMATS)
def test_apply_equals_the_contract(ctx, tile, L, dtype):
    rng = np.random.default_rng(50 + L)
    lo, hi = extremes(dtype)
    dt = np.dtype(dtype).newbyteorder("<")
    mid = 128 if dtype == "uint8" else 0
    for B in BLOCKS:
        for i, F in enumerate(frame_counts(B, tile)):
            K = -(-F // B)
            G = (0, 1, 64)[i % 3]
            # a quiet background (|16 x - dc| <= 16 * 20 + 97: energy <= 2 * 417^2 < 350 000) with placed hits
            x = (mid + rng.integers(-20, 21, (F, L))).astype(dt)
            for f in hit_places(F, B, tile, G):
                x[f, rng.integers(0, L)] = (hi, lo)[f % 2]
            plan = varied_plan(K, 400000)
            want, blanked, _ = same_apply(ctx, x, dtype, L, B, plan, G)
            if F > B + 1000:
                y = want.reshape(F, L).astype(bool).any(axis=1)
                s0 = B + 200                                     # hits 2 G + 1 apart: their blanked runs touch
                assert not y[s0 - G:s0 + 3 * G + 2].any()
                s0 = B + 600                                     # 2 G + 2 apart: one frame between them survives
                assert not y[s0 - G:s0 + G + 1].any() and y[s0 + G + 1] and not y[s0 + G + 2:s0 + 3 * G + 3].any()
            # full-scale data, about one frame in a hundred hit: every window of the dilation sees all kinds of neighbours
            x = random_record(rng, dtype, F * L).reshape(F, L)
            e_hi = (16 * (hi - lo)) ** 2 * L // 4
            same_apply(ctx, x, dtype, L, B, varied_plan(K, int(0.97 * e_hi) if L == 1 else int(0.80 * e_hi)), (64, 0, 1, 7)[i % 4])
    # the same record twice, the input left alone, a window of the output, the timing
    F = 3 * tile + 5
    x = random_record(rng, dtype, F * L)
    plan = varied_plan(-(-F // 272), int((0.97 if L == 1 else 0.80) * ((16 * (hi - lo)) ** 2 * L // 4)))
    want, blanked, clipped = spec.condition(x, dtype, L, 272, plan, 8)
    rec = up(ctx, x)
    try:
        a = ctx.condition(rec, dtype, L, 272, plan, 8)
        b = ctx.condition(rec, dtype, L, 272, plan, 8)
        assert rec.download().tobytes() == x.tobytes()
        assert a.download().tobytes() == want.tobytes() == b.download().tobytes()
        assert (a.blanked, a.clipped) == (b.blanked, b.clipped) == (blanked, clipped) and blanked > 0 and clipped > 0
        assert a.download(L * tile - 3, 11).tobytes() == want[L * tile - 3:L * tile + 8].tobytes()
        assert ctx.cond_timing()[1] > 0.0
        a.free()
        b.free()
    finally:
        rec.free()


def test_int16_quantiser_is_exhaustive(ctx):
    """All 65 536 values at every (mult, shift) and DC of the list; the rounding ties of either sign."""
    x = np.arange(-32768, 32768).astype("<i2")
    shuffled = np.random.default_rng(51).permutation(x)
    K = 65536 // 256
    for mult, shift in ((1, 0), (32767, 0), (32767, 30), (16384, 10)):
        for dc in (0, 7, -7, 1 << 19, -(1 << 19)):
            plan = np.zeros(K, dtype=spec.PLAN_DTYPE)
            plan["dc0"], plan["dc1"], plan["mult"], plan["shift"], plan["theta"] = dc, -dc, mult, shift, spec.INT64_MAX
            a, blanked, _ = same_apply(ctx, x, "int16", 1, 256, plan, 64)
            b, _, _ = same_apply(ctx, shuffled, "int16", 2, 256, plan[:K // 2], 0)
            assert blanked == 0 and (dc != 0 or np.array_equal(np.sort(a), np.sort(b)))
    # (1, 0) with dc = -8: y = (16 x + 8 + 8) >> 4 = x + 1, a tie at every x, rounded up on either side of zero;
    # dc = 8: (16 x - 8 + 8) >> 4 = x;  (3, 1) with dc = 0: (48 x + 16) >> 5, ties at odd x: -3 -> -4, -1 -> -1, 1 -> 2, 3 -> 5
    v = np.zeros(256, dtype="<i2")
    v[:8] = [-3, -2, -1, 0, 1, 2, 3, 100]
    for dc, mult, shift, head in ((-8, 1, 0, [-2, -1, 0, 1, 2, 3, 4, 101]), (8, 1, 0, [-3, -2, -1, 0, 1, 2, 3, 100]),
                                  (0, 3, 1, [-4, -3, -1, 0, 2, 3, 5, 127])):
        plan = np.zeros(1, dtype=spec.PLAN_DTYPE)
        plan[0] = (dc, 0, mult, shift, spec.INT64_MAX)
        y, _, _ = same_apply(ctx, v, "int16", 1, 256, plan, 0)
        assert list(y[:8]) == head, (dc, mult, shift, list(y[:8]))


def test_refusals_on_the_device(ctx):
    n = pkg()._native
    rec = ctx.upload(np.zeros(1000, dtype=np.int8))
    odd = ctx.upload(np.zeros(1001, dtype=np.int8))
    try:
        good = np.zeros(4, dtype=spec.PLAN_DTYPE)
        good["mult"] = 1
        for r, dt, L in ((odd, "int8", 2), (odd, "int16", 1), (rec, "int16", 2)):
            if r is rec:
                continue
            for call in (lambda: ctx.cond_stats(r, dt, L, 256, 256), lambda: ctx.condition(r, dt, L, 256, good, 8)):
                with pytest.raises(n.SgxError) as e:
                    call()
                assert e.value.code == n.SGX_E_ARG and "whole frames" in str(e.value)
        with pytest.raises(n.SgxError) as e:                       # 1002 bytes of int16 pairs: 250.5 frames
            ctx.cond_stats(ctx.upload(np.zeros(1002, dtype=np.int8)), "int16", 2, 256, 256)
        assert e.value.code == n.SGX_E_ARG and "whole frames" in str(e.value)
        with pytest.raises(n.SgxError) as e:
            ctx.cond_stats(rec, "int16", 1, 256, 256, offset_binary=True)
        assert e.value.code == n.SGX_E_ARG and "OFFSET_BINARY" in str(e.value)
        for bad_plan in (good[:3], np.zeros(5, dtype=spec.PLAN_DTYPE)):
            with pytest.raises(n.SgxError) as e:
                ctx.condition(rec, "int8", 1, 256, bad_plan, 8)
            assert e.value.code == n.SGX_E_ARG and "plan" in str(e.value)
        for field, v in (("mult", 0), ("shift", 31), ("dc0", (1 << 20) + 1), ("theta", -1)):
            bad = good.copy()
            bad[field][2] = v
            with pytest.raises(n.SgxError) as e:
                ctx.condition(rec, "int8", 1, 256, bad, 8)
            assert e.value.code == n.SGX_E_ARG and "plan entry 2" in str(e.value)
        for kw in (dict(block=255), dict(block=16400), dict(block=264), dict(lanes=3), dict(guard=65)):
            a = dict(lanes=1, block=256, guard=8)
            a.update(kw)
            with pytest.raises(n.SgxError) as e:
                ctx.condition(rec, "int8", a["lanes"], a["block"], good, a["guard"])
            assert e.value.code == n.SGX_E_ARG
        with pytest.raises(n.SgxError) as e:
            ctx.cond_stats(rec, "int8", 1, 256, 15)
        assert e.value.code == n.SGX_E_ARG and "blank_q4" in str(e.value)
        out = ctx.condition(rec, "int8", 1, 256, good, 8)           # and the good call goes through
        assert len(out) == 1000 and (out.blanked, out.clipped) == (0, 0) and not out.download().any()
        out.free()
    finally:
        odd.free()
        rec.free()


# ---- end to end --------------------------------------------------------------------------------------------------------------

def _same_search(a, ref):
    assert np.array_equal(a.codePhase, ref["codePhase"])
    assert np.array_equal(a.carrFreq, ref["carrFreq"])
    assert np.array_equal(np.asarray(a.internals["freqBin"]), ref["freqBin"])
    assert np.allclose(a.peakMetric, ref["peakMetric"], rtol=1e-9, atol=0)


def test_post_processing_of_the_stepped_capture(tmp_path):
    m = pkg()
    x = cases.capture()
    path = tmp_path / "stepped_sc16.bin"
    x.tofile(str(path))
    s = SCENE.settings(m, msToProcess=float(TRK_MS), dataType="int16", frontEndConditioning=True)
    acq, trk, nav = s.postProcessing(str(path))
    assert nav is None or nav._solutions is None                               # 300 ms carry no subframe
    info = dict(s.lastConditioning)
    count = info["samples"]
    n = SCENE.samples_per_code
    assert TRK_MS * n < count <= x.size and count % 2 == 0
    assert (info["block"], info["blank_q4"]) == (cases.BLOCK, cases.BLANK_Q4)
    assert s.iqRecord and s.dataType == "int16" and s.frontEndConditioning                           # left alone
    assert acq.settings.dataType == 'int8' and not acq.settings.iqRecord and acq.settings.skipNumberOfBytes == 0
    st, plan, y8, blanked, clipped = cases.conditioned(x[:count])
    assert info["blocks"] == plan.size
    assert info["blanked"] == blanked / (count // 2) and info["clipped"] == clipped / count
    gain_db = 20.0 * np.log10(plan["mult"] / np.exp2(plan["shift"].astype(np.float64)))
    assert abs(info["gain_db_min"] - gain_db.min()) < 1e-9 and abs(info["gain_db_max"] - gain_db.max()) < 1e-9
    assert info["gain_db_max"] - info["gain_db_min"] > 17.0                    # the 18 dB step was followed
    assert info["dc_max"] == (plan["dc0"].max() / 16.0, plan["dc1"].max() / 16.0)
    want = cases.convert(y8)
    with s._prepared_record(str(path), 0, count) as rec:
        assert rec.download().tobytes() == want.tobytes()                      # the contracts' record, byte for byte
    o = SCENE.oracle_settings(msToProcess=float(TRK_MS))
    ref = orc.acquire(o, want[:11 * n])
    _same_search(acq, ref)
    assert sorted(np.flatnonzero(acq.carrFreq) + 1) == sorted(SCENE.prns)
    chans = orc.pre_run(o, ref)
    assert np.array_equal(acq.channels.PRN, chans["PRN"]) and np.count_nonzero(acq.channels.PRN) == len(SCENE.prns)
    same_tracking(trk, orc.stack_series(orc.track(o, chans, want)), len(SCENE.prns), TRK_MS)


def test_a_real_int16_record_is_tracked_by_trk3_after_conditioning(tmp_path):
    m = pkg()
    x = cases.real_int16(TRK_MS + 4)
    path = tmp_path / "real_int16.bin"
    x.tofile(str(path))
    s = m.Settings()
    s.samplingFreq, s.IF, s.dataType, s.numberOfChannels = cases.REAL_FS, cases.REAL_IF, "int16", cases.REAL_SATS
    s.msToProcess, s.frontEndConditioning = float(TRK_MS), True
    acq, trk, nav = s.postProcessing(str(path))
    assert nav is None or nav._solutions is None
    info = dict(s.lastConditioning)
    count = info["samples"]
    block = spec.block_frames(cases.REAL_FS, cases.BLOCK_US)
    assert info["block"] == block and TRK_MS * 38192 < count <= x.size
    assert acq.settings.dataType == 'int8' and s.dataType == 'int16'
    ctx = m.engine.get_context(acq.settings, None)
    assert m._native.track_plan(acq.settings, m._native.DT_INT8, cases.REAL_SATS)[0] == 5            # trk3_kernel
    assert ctx.timing()["track_kernel"] == 5
    st, plan, want, blanked, clipped = cases.conditioned(x[:count], 1, block)
    assert info["blanked"] == blanked / count and info["clipped"] == clipped / count
    with s._prepared_record(str(path), 0, count) as rec:
        assert rec.download().tobytes() == want.tobytes()
    o = orc.OracleSettings(samplingFreq=cases.REAL_FS, IF=cases.REAL_IF, numberOfChannels=cases.REAL_SATS,
                           msToProcess=float(TRK_MS))
    ref = orc.acquire(o, want[:11 * 38192])
    _same_search(acq, ref)
    assert sorted(np.flatnonzero(acq.carrFreq) + 1) == sorted(SCENE.prns[:cases.REAL_SATS])
    chans = orc.pre_run(o, ref)
    same_tracking(trk, orc.stack_series(orc.track(o, chans, want)), cases.REAL_SATS, TRK_MS)
