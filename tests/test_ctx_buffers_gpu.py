"""The context's memory on the GPU (csrc/sgx_internal.h: DevBuf, LookPage, ~sgx_ctx): scratch that has grown for a larger
call serves a smaller one unchanged, a context can be made and destroyed over and over, and the gathered peak records fill
their part of the result page to the last one.  Everything at 4.099 Msps, the lowest rate of tests/any_rate.py (N = 4 099, the
padded search), on contexts of the tests' own (engine.get_context would hand out one that other tests have used).
Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import any_rate
from conftest import pkg
from oracle import softgnss_oracle as orc

pytestmark = pytest.mark.gpu

FS, IF = any_rate.RATES[3]
N = 4099
FOUR = [0, 1, 2, 3]             # the small search: PRNs 1..4, one of them in the record
TWELVE = list(range(12))        # the large one: PRNs 1..12, four of them in the record


def _settings():
    return any_rate.settings(FS, IF)


def _context():
    return pkg()._native.Context(_settings(), 0)


@pytest.fixture(scope="module")
def four_sat_record():
    """12 ms with PRNs 2, 5, 9 and 12 (peakMetric 7.8 .. 19 in the 1-ms search, 22 .. 30 in the 2-ms one; every other PRN
    below 1.9 against the threshold of 2.5)."""
    synth = pkg("synth")
    sc = synth.Scene.make(0xB0F0000 + N, FS, IF, [2, 5, 9, 12], [1750.0, -3300.0, 400.0, -900.0], [N // 3, N - 5, 17, N // 2],
                          [9, 8, 9, 8])
    x = synth.generate(sc, synth.record_length(N, 12))
    x.setflags(write=False)
    return x


def _small_search(ctx, rec):
    return ctx.acquire(rec, 0, 11 * N, FOUR)


def _same(a, b):
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def test_acquisition_scratch_serves_a_smaller_search_after_a_larger_one(four_sat_record):
    """A 1-ms search over 4 PRNs (58 rows per PRN, one detection: one fine row), a coherent 2 x 2 ms search over 12 PRNs (114
    rows per PRN, four detections: two fine rows), the first search again: the first and the third equal bit for bit, and
    equal the same search on a context that has run nothing else."""
    ctx, fresh = _context(), _context()
    try:
        rec = ctx.upload(four_sat_record)
        first = _small_search(ctx, rec)
        large = ctx.acquire_coherent(rec, 0, 12 * N, TWELVE, coherent_ms=2, n_windows=2)
        third = _small_search(ctx, rec)
        alone = _small_search(fresh, fresh.upload(four_sat_record))
    finally:
        ctx.close()
        fresh.close()
    assert list(first["carrFreq"] > 0) == [False, True, False, False]
    assert [p + 1 for p in TWELVE if large["carrFreq"][p] > 0] == [2, 5, 9, 12]
    _same(first, third)
    _same(first, alone)


def _chans(n_ch):
    """n_ch channels on the two satellites of any_rate.record: (PRN, acquiredFreq, codePhase)."""
    two = [(2, IF + 1750.0, float(N // 3)), (5, IF - 3300.0, float(N - 5))]
    return [two[i % 2] for i in range(n_ch)]


def _track_pageable(ctx, rec, n_ch, ms):
    """sgx_track_ex with a plain numpy result buffer: the series come through the context's device staging buffer."""
    n = pkg()._native
    arr = n._chan_array(_chans(n_ch))
    out = np.full((n_ch, n.NUM_SERIES, ms), -1.0)
    done = np.full(n_ch, -1, dtype=np.int32)
    n.check(n.lib().sgx_track_ex(ctx._h, rec._h, 0, C.cast(arr, C.c_void_p), n_ch, ms, n._ptr(out), n._ptr(done), n.DT_INT8))
    return out, done


def test_tracking_scratch_on_the_pageable_path_serves_a_smaller_call_after_a_larger_one():
    """1 channel x 4 ms, 9 channels x 8 ms, 1 channel x 4 ms through a pageable result buffer: the first and the third equal
    bit for bit and equal a fresh context's; the 9-channel run equals Context.track's, whose buffer is pinned."""
    host = any_rate.record(FS, IF)
    ctx, fresh = _context(), _context()
    try:
        rec = ctx.upload(host)
        first = _track_pageable(ctx, rec, 1, 4)
        nine = _track_pageable(ctx, rec, 9, 8)
        third = _track_pageable(ctx, rec, 1, 4)
        pinned = ctx.track(rec, _chans(9), 8)
        alone = _track_pageable(fresh, fresh.upload(host), 1, 4)
    finally:
        ctx.close()
        fresh.close()
    assert list(first[1]) == [4] and list(nine[1]) == [8] * 9
    for other in (third, alone):
        assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1])
    assert np.array_equal(nine[0], pinned[0]) and np.array_equal(nine[1], pinned[1])


def test_twenty_contexts_in_a_row(four_sat_record):
    """Create, use (one upload, one small search) and destroy a context twenty times in one process: the last search equals
    the first bit for bit."""
    results = []
    for _ in range(20):
        ctx = _context()
        try:
            results.append(_small_search(ctx, ctx.upload(four_sat_record)))
        finally:
            ctx.close()
    assert np.sum(results[0]["carrFreq"] > 0) == 1
    _same(results[0], results[-1])


@pytest.fixture(scope="module")
def all_prns_oracle(four_sat_record):
    o = orc.OracleSettings(samplingFreq=FS, IF=IF, acqSatelliteList=list(range(1, 33)), numberOfChannels=2, msToProcess=50.0)
    return orc.acquire(o, four_sat_record[:11 * N])


# 32 PRNs over 25 ranks are 2 slots each: 50 records, the most the page's gather part holds (26 ranks: 52)
@pytest.mark.parametrize("world,ranks", [(1, [0]), (25, [0, 6, 7, 24])])
def test_sharded_gather_without_a_communicator(world, ranks, four_sat_record, all_prns_oracle):
    """sgx_acquire_sharded with no communicator, each rank's shard run alone: its own PRNs to the bars of
    tests/test_any_rate_gpu.py against oracle.acquire, every other entry at its reset value."""
    sh = pkg("shard")
    ref = all_prns_oracle
    assert [p + 1 for p in range(32) if ref["carrFreq"][p] > 0] == [2, 5, 9, 12]
    ctx = _context()
    try:
        rec = ctx.upload(four_sat_record)
        got = {rank: ctx.acquire_sharded(None, rank, world, rec, 0, 11 * N) for rank in ranks}
    finally:
        ctx.close()
    for rank, g in got.items():
        mine = list(sh.plan_shards(32, world)[rank])
        other = [p for p in range(32) if p not in mine]
        for f in ("codePhase", "carrFreq", "freqBin", "fineIdx"):
            assert np.array_equal(g[f][mine], ref[f][mine]), (rank, f)
        assert np.allclose(g["peakMetric"][mine], ref["peakMetric"][mine], rtol=1e-9, atol=0), rank
        for f, reset in (("carrFreq", 0.0), ("codePhase", 0.0), ("peakMetric", 0.0), ("freqBin", -1), ("fineIdx", -1)):
            assert np.all(g[f][other] == reset), (rank, f)
