"""The helpers of tests/big_record.py without a GPU: their arithmetic at a small boundary against the numpy contracts run by
brute force on the whole small record, the wrap rule on every window of tests/test_big_record_gpu.py at B = 2^32 - and that
the rule rejects a block of 2^20 bytes, which divides both boundaries -, the host generator across 2^31 and 2^32, the
oracle's indifference to where its window starts, and the cancellation's windows (big.CancelPlan) against its contract and
its host twin on the whole small record."""
import numpy as np
import pytest

import big_record as big
import cond_spec
import waterfall_spec
from conftest import pkg
from oracle_helpers import oracle_channel

SMALL_B, SMALL_P, SMALL_EXTRA = 1 << 16, 105 << 3, 48 * 20


@pytest.fixture(scope="module")
def small():
    rec = big.Tiled(SMALL_B, SMALL_P, SMALL_EXTRA)
    cases = big.stage_cases(rec, small=True)
    cases.update(big.small_cond_cases())
    return rec, cases


NAMES = sorted(big.stage_cases(big.Tiled(SMALL_B, SMALL_P, SMALL_EXTRA), small=True)) + ["condition_int8", "condition_int16"]


def test_the_tiled_record_is_what_its_reader_says():
    rec = big.Tiled(SMALL_B, SMALL_P, SMALL_EXTRA)
    b = rec.build()
    assert b.size == rec.n == SMALL_B + SMALL_EXTRA == rec.reps * rec.P + rec.rest
    assert np.array_equal(b, rec.at(0, rec.n)) and np.array_equal(rec.at(-5, 3), np.r_[rec.block[-5:], rec.block[:3]])
    for k in (2, 3):
        assert np.array_equal(rec.model(k), np.r_[b[:k * rec.P], b[rec.reps * rec.P:]])
    for a, c in ((0, rec.n), (17, SMALL_B + 3), (SMALL_B - 1, SMALL_B + 1), (5, 5)):
        v = b[a:c].astype(np.int64)
        m, h = rec.sums(a, c)
        assert m == [v.size, int(v.sum()), int((v ** 2).sum()), int((v ** 4).sum())]
        assert np.array_equal(h, np.bincount(v + 128, minlength=256))
    # the full-size block obeys what the stages' framing asks of it and divides neither boundary
    full = big.P32
    assert all(full % (16 * M) == 0 for M in (1, 2, 3)) and full % 8 == 0 and full % (16 * 16) == 0
    assert full % (8192 * 1 * 1) == 0 and full % (2048 * 2 * 2) == 0                      # the conditioning cases' blocks
    assert (1 << 31) % full and (1 << 32) % full and big.EXTRA32 % 48 == 0


@pytest.mark.parametrize("name", NAMES)
def test_tiled_expectations_equal_the_contract_by_brute_force(small, name):
    """At the small boundary the windows (first, across B / 2 and B on either side of the stage, last) and the whole-record
    counters first + (reps - 2) middle + last equal the stage's numpy contract on the whole record."""
    stage, rec = small[1][name]
    whole, counted = stage.run(rec.build(), 0)
    assert whole.size == stage.out_len(rec.n)
    windows = stage.windows(rec, 64)
    assert len(windows) >= 4 and windows[0] == (0, 64) and windows[-1][1] == whole.size
    assert any(w0 < stage.out_of(rec.B) < w1 for w0, w1 in windows) or stage.out_of(rec.B) > whole.size
    for w0, w1 in windows:
        assert stage.window(rec.at, rec.n, w0, w1).tobytes() == whole[w0:w1].tobytes(), (name, w0, w1)
    assert stage.counters(rec) == counted, name
    assert all(0 < v for k, v in counted.items() if k in ("clipped", "blanked")), counted
    assert counted.get("clipped", 1) < whole.size
    if name.startswith("requantize"):
        x = big.requant_spec.elements(rec.build(), stage.dtype)
        assert stage.max_abs(rec) == float(np.abs(x[np.isfinite(x)].astype(np.float64)).max())
        a, c = (rec.B // 2) // stage.den - 100, rec.B // stage.den + 77                  # an element window across B
        part = big.requant_counts(rec.at(a * stage.den, c * stage.den), stage.dtype)
        assert part == big.requant_counts(rec.build()[a * stage.den:c * stage.den], stage.dtype)
    if name.startswith("condition"):
        assert np.array_equal(stage.record_stats(rec),
                              cond_spec.block_stats(rec.build(), stage.dtype, stage.lanes, stage.block, stage.blank_q4))
        assert stage.record_plan(rec).size == -(-rec.n // stage.unit)


def test_the_monitor_s_whole_record_expectation_equals_the_contract():
    rec = big.Tiled(SMALL_B, SMALL_P, SMALL_EXTRA)
    N, tail, fs = 256, 100, 38.192
    got = big.waterfall_whole(rec, N, tail, fs)
    want = waterfall_spec.waterfall(rec.build(), 0, SMALL_B + N + tail, fs, N, 0, SMALL_B)
    assert got["phases"] == rec.P // np.gcd(rec.P, N) == 105
    for k in ("moments", "hist", "n_segments"):
        assert np.array_equal(got[k], want[k]), k
    # the same spectra summed phase by phase instead of segment by segment: rounding of 256 additions
    assert np.abs(got["pxx"] - want["pxx"]).max() < 1e-12 * want["pxx"].max()


def test_the_cancellation_s_windows_equal_the_contract_and_the_host_twin_on_the_whole_record():
    """big.CancelPlan at B = 2^20: every window obeys the rule, the windows of the contract on the WHOLE small record with all
    four channels are the windows' own expectations (bytes, v and counts), the quiet windows and everything between the
    windows are the input, and sgx_cancel_host on the whole record equals the windows under the rule of
    cancel_cases.compare, its clip count the sum of theirs."""
    n = pkg("_native")
    B = 1 << 20
    rec = big.Tiled(B, 105 << 10, extra=48 * 700 + 5)
    plan = big.CancelPlan(rec)
    x = rec.build()
    assert rec.n % 16 != 0 and [plan.BLOCKS[k] for k in plan.names] == list(plan.ms_done) and plan.s.samplingFreq == 2.046e6
    whole = big.cancel_spec.cancel(plan.s, x, 0, plan.chans, plan.series, plan.ms_done, plan.amp)
    y, clipped = n.cancel_host(plan.s, x, plan.chans, plan.series, plan.amp, ms_done=plan.ms_done)
    total, inside = 0, np.zeros(rec.n, dtype=bool)
    for i, (w0, w1) in enumerate(plan.windows):
        assert w1 - w0 >= plan.BLOCKS[plan.names[i]] * 2045 + (plan.MARGIN if i in (2, 3) else 2 * plan.MARGIN)
        want = big.wrap_visible(rec.at, plan.contract(i), (w0, w1), B=B)
        exp = plan.expect(rec.at, i, w0, w1)
        assert want.tobytes() == exp[0].tobytes() == whole[0][w0:w1].tobytes() and np.any(want != x[w0:w1])
        assert np.array_equal(exp[1], whole[1][w0:w1]) and np.array_equal(exp[3], whole[3][w0:w1])
        assert 0 < exp[2] < exp[3].sum() and exp[3].sum() >= plan.BLOCKS[plan.names[i]] * 2045
        big.cancel_cases.compare_to(exp, plan.names[i], y[w0:w1])
        total += exp[2]
        inside[w0:w1] = True
    assert whole[2] == total == clipped and not whole[3][~inside].any()
    assert np.array_equal(y[~inside], x[~inside])
    for w0, w1 in plan.quiet:
        assert not inside[w0:w1].any() and w1 - w0 > 2 * 4096
        want = big.wrap_visible(rec.at, big.identity, (w0, w1), B=B)
        assert y[w0:w1].tobytes() == want.tobytes() == whole[0][w0:w1].tobytes()
    # the plan of the GPU test: the same placement at 2^32, block 2 of channel B on a tile's first sample past 2^32 - 1
    full = big.CancelPlan(big.Tiled())
    assert int(full.series[1, 0, 1]) == big.B32 and big.B32 % 4096 == 0 and int(full.series[2, 0, 3]) == big.B32 + big.EXTRA32
    assert full.quiet[0][0] < big.B32 // 2 + (1 << 20) < full.quiet[0][1]
    assert full.quiet[1][0] < big.B32 - (1 << 20) < full.quiet[1][1]
    for i, w in enumerate(full.windows):
        big.wrap_visible(full.rec.at, full.contract(i), w)
    for w in full.quiet:
        big.wrap_visible(full.rec.at, big.identity, w)


# ---- the wrap rule ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiled():
    return big.Tiled()


def test_every_stage_window_of_the_gpu_test_obeys_the_rule(tiled):
    assert tiled.n == big.B32 + big.EXTRA32
    checked = 0
    for name, (stage, rec) in sorted(big.stage_cases(tiled).items()):
        windows = stage.windows(rec)
        assert len(windows) >= 4, name
        for w in windows:
            big.wrap_visible(rec.at, stage.contract(rec.n), w)
            checked += 1
    assert checked >= 4 * 9
    # the handle's windows, the monitor's kept slice and its second call read the bytes as they are
    for w in ((0, 4096), (big.B32 // 2 - 2048, big.B32 // 2 + 2048), (big.B32 - 2048, big.B32 + 2048), (tiled.n - 4096, tiled.n),
              (big.B32, big.B32 + big.WF_SEGMENT + big.WF_TAIL), (big.WF_SECOND[0], big.WF_SECOND[0] + big.WF_SECOND[1])):
        big.wrap_visible(tiled.at, big.identity, w)


def test_the_rule_rejects_a_block_that_divides_the_boundary():
    """The mutation: a block of 2^20 bytes.  Byte p and byte p - 2^32 are the same byte, and a wrapped address reads it."""
    blind = big.Tiled(P=1 << 20)
    stage = big.Decim(16, 31)
    for w in stage.windows(blind)[1:-1]:
        with pytest.raises(AssertionError, match="give the same bytes"):
            big.wrap_visible(blind.at, stage.contract(blind.n), w)
    with pytest.raises(AssertionError, match="give the same bytes"):
        big.wrap_visible(blind.at, big.identity, (big.B32 - 100, big.B32 + 100))
    # ... while the block that is used passes the same windows
    good = big.Tiled()
    for w in stage.windows(good):
        big.wrap_visible(good.at, stage.contract(good.n), w)


def test_scene_and_sparse_windows_obey_the_rule():
    synth = pkg("synth")
    sc = synth.Scene.default()
    at = big.scene_reader(synth.generate, sc)
    for name, (w0, w1) in sorted(big.scene_windows().items()):
        assert 0 <= w0 < w1 <= big.SCENE_N, name
        big.wrap_visible(at, big.identity, (w0, min(w1, w0 + big.PROBE_RULE)))
    assert big.TRACK_WINDOW[0] < big.B32 < big.TRACK_WINDOW[1] and big.ACQ_WINDOW[0] < big.B32 < big.ACQ_WINDOW[1]
    low = big.scene_reader(synth.generate, synth.Scene.make(*big.LOW_SCENE))              # the low-rate scene made on the device
    w0, w1 = big.low_rate_window()
    assert 0 < w0 < big.B32 < w1 <= big.LOW_N
    big.wrap_visible(low, big.identity, (w0, w0 + big.PROBE_RULE))
    # the coherent run on that window: the boundary lies in its pull-in, and what its groups read - all of it beyond 2^32 -
    # obeys the rule as well
    c0, c1 = big.low_rate_coherent_window()
    assert w0 + big.LOW_COHERENT["P"] * (big.LOW_SPC - 1) > big.B32 > w0 + 11 * big.LOW_SPC and big.B32 < c0 < c1 <= w1
    assert c0 + big.PROBE_RULE <= c1
    big.wrap_visible(low, big.identity, (c0, c0 + big.PROBE_RULE))
    # the typed sparse records: the payload starts 20 code periods (of its sample width) before byte 2^32
    for isz, spc in ((2, big.SPC), (4, big.SPC), (1, big.LOW_SPC)):
        start, nbytes = big.typed_start(isz, spc), (big.TRACK_MS + 13) * spc * isz
        assert start < big.B32 < start + nbytes
        sp = big.sparse_reader(start + nbytes, start, np.full(nbytes, 9, dtype=np.int8), 128 if isz == 1 else 0)
        big.wrap_visible(sp, big.identity, (start, start + big.PROBE_RULE), sparse=True)
    # a sparse record: the payload in the last window, the filler everywhere else
    payload = np.arange(1, 5001, dtype=np.int16)
    n = big.B32 + payload.nbytes
    for fill in (0, 128):
        sp = big.sparse_reader(n, big.B32, payload, fill)
        assert sp(big.B32 - 2, big.B32 + 4).view(np.uint8).tolist() == [fill, fill, 1, 0, 2, 0]
        with pytest.raises(AssertionError, match="two wrapped readings"):     # both find the filler, nothing else
            big.wrap_visible(sp, big.identity, (big.B32, n))
        assert big.wrap_visible(sp, big.identity, (big.B32, n), sparse=True).tobytes() == payload.tobytes()
        with pytest.raises(AssertionError, match="give the same bytes"):      # a window of filler shows nothing
            big.wrap_visible(sp, big.identity, (big.B32 - 5000, big.B32 - 10), sparse=True)
    # the file's written windows: random bytes in a hole of zeros
    for w0, w1 in big.FILE_WINDOWS:
        sp = big.sparse_reader(big.B32 + big.FILE_TAIL, w0, np.full(w1 - w0, 7, dtype=np.int8))
        big.wrap_visible(sp, big.identity, (w0, w1), sparse=True)


# ---- the host generator and the oracle ----------------------------------------------------------------------------------

def test_the_host_generator_is_consistent_across_the_boundaries():
    synth = pkg("synth")
    sc = synth.Scene.default()
    for X in (1 << 31, 1 << 32):
        whole = synth.generate(sc, 3000, offset=X - 1000)
        assert np.array_equal(whole[:1000], synth.generate(sc, 1000, offset=X - 1000))
        assert np.array_equal(whole[1000:], synth.generate(sc, 2000, offset=X))
        assert np.array_equal(whole[999:1002], synth.generate(sc, 3, offset=X - 1))
        assert np.array_equal(whole, synth.generate(sc, 3000, offset=X - 1000, chunk=999))     # the chunk seams move
        assert whole.std() > 10 and not np.array_equal(whole, synth.generate(sc, 3000, offset=X // 2 - 1000))


def test_the_oracle_does_not_care_where_its_window_starts():
    """oracle_channel on a window that starts at W0, code phase cp - W0, and on one that starts a code period earlier: the
    same series, absoluteSample shifted by exactly the difference.  The GPU test adds W0 to the oracle's absoluteSample."""
    synth = pkg("synth")
    sc = synth.Scene.default()
    sat = sc.sats[0]
    ms, W0 = 5, big.TRACK_START
    cp = big.first_code_start(sat, W0 + 100)
    assert W0 + 100 <= cp < W0 + 100 + big.SPC + 1
    host = synth.generate(sc, (ms + 3) * big.SPC, offset=W0 - big.SPC)
    freq = 9548000.0 + 1250.0
    late = oracle_channel((host[big.SPC:], sat["prn"], freq, float(cp - W0), ms))
    early = oracle_channel((host, sat["prn"], freq, float(cp - W0 + big.SPC), ms))
    assert np.array_equal(early[0], late[0] + big.SPC) and np.array_equal(early[1:], late[1:])
    assert np.all(np.diff(late[0]) >= big.SPC - 1) and np.hypot(late[3], late[7]).mean() > 20000.0        # on the code
