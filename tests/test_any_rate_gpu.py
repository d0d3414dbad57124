"""Acquisition on the GPU at sampling rates whose samplesPerCode has a prime factor above 31 (53, 37, 5.714 and 4.099
Msps): csrc/sgx_acq.hip runs the search on a padded length (acquire_passes).  Every entry point against oracle.acquire to
the bars of tests/test_gpu_parity.py - codePhase, freqBin, fineIdx and carrFreq exactly, peakMetric within 1e-9 relative -
then preRun and 50 ms of tracking; the code-phase edges of acq_edges.npz restated for N = 5 714; the coherent direct path
against the numpy contract.  tests/any_rate.py holds the cases, tests/test_any_rate_host.py conditions each of them in
numpy.  Run with -m gpu."""
import numpy as np
import pytest

import any_rate
import dense_child
from conftest import pkg
from oracle import softgnss_oracle as orc
from test_coherent_acq_gpu import _dense_compare

pytestmark = pytest.mark.gpu

TRK_TOL = 1e-6
IDX = [p - 1 for p in any_rate.PRNS]


def _trk_err(got, want):
    errs = []
    for c in range(want.shape[0]):
        scale = max(1.0, float(np.sqrt(np.mean(want[c, 3] ** 2 + want[c, 7] ** 2))))
        errs.append(np.max(np.abs(got[c, 3:9] - want[c, 3:9])) / scale)
    return max(errs)


def _same_search(a, ref, idx=IDX):
    """An AcquisitionResult against oracle.acquire's dict, on the searched PRN indices and on the untouched rest."""
    assert np.array_equal(a.codePhase, ref["codePhase"])
    assert np.array_equal(a.carrFreq, ref["carrFreq"])
    assert np.array_equal(np.asarray(a.internals["freqBin"])[idx], ref["freqBin"][idx])
    assert np.array_equal(np.asarray(a.internals["fineIdx"])[idx], ref["fineIdx"][idx])
    assert np.allclose(a.peakMetric, ref["peakMetric"], rtol=1e-9, atol=0), (a.peakMetric[idx], ref["peakMetric"][idx])


def _equal_results(a, b):
    for f in ("carrFreq", "codePhase", "peakMetric"):
        assert np.array_equal(a.results[f], b.results[f]), f
    for f in ("freqBin", "fineIdx"):
        assert np.array_equal(a.internals[f], b.internals[f]), f


def test_the_rates_are_the_padded_ones():
    m = pkg()
    for fs, IF in any_rate.RATES:
        n = any_rate.settings(fs, IF).samplesPerCode
        assert m._native.acquire_fft_length(n) >= 2 * n - 1


@pytest.mark.parametrize("fs,IF", any_rate.RATES, ids=any_rate.RATE_IDS)
def test_front_ends_that_do_not_factor_against_oracle(fs, IF):
    """The scene of test_other_front_ends_against_oracle: acquisition, preRun and 50 ms of tracking."""
    m = pkg()
    s, o = any_rate.settings(fs, IF), any_rate.oracle_settings(fs, IF)
    n = s.samplesPerCode
    assert n == int(round(fs / 1000))
    rec_host = any_rate.record(fs, IF)
    a = m.AcquisitionResult(s, device=0)
    a.acquire(rec_host[:11 * n])
    ref = orc.acquire(o, rec_host[:11 * n])
    _same_search(a, ref)
    assert [p + 1 for p in range(32) if a.carrFreq[p] > 0] == [2, 5]
    a.preRun()
    chans_ref = orc.pre_run(o, ref)
    assert np.array_equal(a.channels.PRN, chans_ref["PRN"])
    assert sorted(int(p) for p in a.channels.PRN) == [2, 5]
    t = m.TrackingResult(a, device=0)
    rec = m.engine.get_context(s, 0).upload(rec_host)
    try:
        t.track(m.DeviceFile(rec))
    finally:
        rec.free()
    want = orc.stack_series(orc.track(o, chans_ref, rec_host))
    assert np.array_equal(t.series[:, 0], want[:, 0])
    assert _trk_err(t.series, want) < TRK_TOL


def test_noncoherent_sum_over_ten_blocks():
    m = pkg()
    fs, IF = any_rate.RATES[2]
    s, o = any_rate.settings(fs, IF), any_rate.oracle_settings(fs, IF)
    x = any_rate.record(fs, IF)[:20 * s.samplesPerCode]
    a = m.AcquisitionResult(s, device=0)
    a.acquire(x, n_blocks=10, noncoh=True)
    _same_search(a, orc.acquire(o, x, n_blocks=10, noncoh=True))
    assert np.sum(a.carrFreq > 0) == 2


def test_float64_signal():
    m = pkg()
    fs, IF = any_rate.RATES[3]
    s, o = any_rate.settings(fs, IF), any_rate.oracle_settings(fs, IF)
    x = any_rate.scaled(any_rate.record(fs, IF)[:11 * s.samplesPerCode])
    a = m.AcquisitionResult(s, device=0)
    a.acquire(x)
    _same_search(a, orc.acquire(o, x))
    assert np.sum(a.carrFreq > 0) == 2


def test_record_offset_that_is_not_a_multiple_of_16():
    m = pkg()
    fs, IF = any_rate.RATES[1]
    s, o = any_rate.settings(fs, IF), any_rate.oracle_settings(fs, IF)
    n = s.samplesPerCode
    host = any_rate.record(fs, IF)
    rec = m.engine.get_context(s, 0).upload(host[:any_rate.OFFSET + 11 * n])
    try:
        a = m.AcquisitionResult(s, device=0)
        a.acquire(m.DeviceSignal(rec, any_rate.OFFSET, 11 * n))
    finally:
        rec.free()
    _same_search(a, orc.acquire(o, host[any_rate.OFFSET:any_rate.OFFSET + 11 * n]))
    assert np.sum(a.carrFreq > 0) == 2


def test_deferred_search_and_queued_step_equal_the_eager_ones():
    m = pkg()
    fs, IF = any_rate.RATES[2]
    s = any_rate.settings(fs, IF)
    n = s.samplesPerCode
    ctx = m.engine.get_context(s, 0)
    rec = ctx.upload(any_rate.record(fs, IF))
    try:
        # the pair itself
        want = ctx.acquire(rec, 0, 11 * n, IDX)
        ctx.acquire_begin(rec, 0, 11 * n, IDX)
        got = ctx.acquire_end(len(IDX))
        assert np.sum(want["carrFreq"] > 0) == 2
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        # acquire -> preRun -> track through the deferred objects
        out = []
        for deferred in (False, True):
            a = m.AcquisitionResult(s, device=0, deferred=deferred)
            a.acquire(m.DeviceSignal(rec, 0, 11 * n))
            a.preRun()
            t = m.TrackingResult(a, device=0)
            t.track(m.DeviceFile(rec))
            out.append((a, t))
        (ae, te), (ad, td) = out
        assert np.array_equal(td.series, te.series)
        _equal_results(ad, ae)
        for f in ("PRN", "acquiredFreq", "codePhase", "status"):
            assert np.array_equal(ad.channels[f], ae.channels[f]), f
        assert sorted(int(p) for p in ae.channels.PRN) == [2, 5]
    finally:
        rec.free()


def test_two_prn_shards_without_a_communicator_equal_the_whole_search():
    m = pkg()
    sh = pkg("shard")
    fs, IF = any_rate.RATES[3]
    s = any_rate.settings(fs, IF)
    n = s.samplesPerCode
    rec = m.engine.get_context(s, 0).upload(any_rate.record(fs, IF)[:11 * n])
    try:
        sig = m.DeviceSignal(rec, 0, 11 * n)
        whole = m.AcquisitionResult(s, device=0)
        whole.acquire(sig)
        parts = []
        for rank in range(2):
            a = m.AcquisitionResult(s, device=0)
            sh.acquire_sharded(a, sig, rank, 2, sh.LocalGather())
            parts.append(a)
    finally:
        rec.free()
    assert np.sum(whole.carrFreq > 0) == 2
    for rank, a in enumerate(parts):
        mine = list(sh.plan_shards(len(IDX), 2)[rank])
        other = [p for p in range(32) if p not in mine]
        for f in ("carrFreq", "codePhase", "peakMetric"):
            assert np.array_equal(a.results[f][mine], whole.results[f][mine]), (rank, f)
            assert not np.any(a.results[f][other]), (rank, f)
        for f in ("freqBin", "fineIdx"):
            assert np.array_equal(np.asarray(a.internals[f])[mine], np.asarray(whole.internals[f])[mine]), (rank, f)


@pytest.mark.parametrize("c", any_rate.EDGE_PHASES)
def test_code_phase_edges_on_a_padded_length(c):
    """One satellite whose peak lies at code phase c: both ends of the row (the code row's wrap-around copy, the cut at
    k < N), and every branch of the exclusion list; at c = samples per chip the reference's IndexError."""
    m = pkg()
    s, o = any_rate.edge_settings(oracle=False), any_rate.edge_settings()
    x = any_rate.edge_record(c)
    a = m.AcquisitionResult(s, device=0)
    if c == any_rate.EDGE_SPC:
        with pytest.raises(IndexError):
            orc.acquire(o, x)
        with pytest.raises(IndexError):
            a.acquire(x)
        return
    a.acquire(x)
    ref = orc.acquire(o, x)
    assert ref["codePhase"][0] == c
    _same_search(a, ref, [0])


@pytest.mark.parametrize("name", [c.name for c in any_rate.COHERENT_CASES])
def test_coherent_direct_path_on_a_padded_length(name):
    m = pkg()
    c = any_rate.COHERENT_BY_NAME[name]
    s = m.Settings()
    s.samplingFreq, s.IF, s.acqSearchBand = c.s.samplingFreq, c.s.IF, c.s.acqSearchBand
    plan = m._native.acquire_coherent_plan(s, c.T, c.M, c.noncoh, c.step)
    assert plan["path"] == "direct" and plan["n_bins"] == c.g["n_bins"]
    want = c.reference()
    got = dense_child.run_case(m, c)
    _dense_compare(c, got, want)
