"""Acquisition at sampling rates whose samplesPerCode does not factor into 2..31, without a GPU: the length chooser
through the C-ABI (sgx_acquire_fft_length), the identity the padded search rests on in numpy against oracle.acquire, and
the conditioning of every search tests/test_any_rate_gpu.py asserts exactly (tests/any_rate.py holds the cases): no
asserted arg-max within 1e-6 (relative) of its runner-up, no peakMetric within 1 % of acqThreshold, no case and no PRN
left out.  1e-6 is a condition, three orders above the 1e-9 allowed on peakMetric."""
import numpy as np
import pytest

import any_rate
import coherent_acq_spec as spec
from conftest import pkg
from oracle import softgnss_oracle as orc
from test_coherent_acq_cases import conditioning


def _next_pow2(v):
    m = 1
    while m < v:
        m <<= 1
    return m


def test_lengths_that_factor_are_kept():
    f = pkg()._native.acquire_fft_length
    for n in any_rate.SMOOTH_IN_USE + [52800, 2 ** 17, 31 ** 3]:
        assert any_rate.smooth(n) and f(n) == n, n


def test_padded_lengths_factor_and_hold_the_correlation():
    f = pkg()._native.acquire_fft_length
    rng = np.random.default_rng(0xA17)
    ns = [53000, 37000, 5714, 4099] + list(range(2046, 2201)) + [int(v) for v in rng.integers(2, 70001, 200)]
    padded = 0
    for n in ns:
        m = f(n)
        if any_rate.smooth(n):
            assert m == n, n
            continue
        padded += 1
        assert m >= 2 * n - 1 and any_rate.smooth(m) and m <= _next_pow2(2 * n - 1), (n, m)
    assert padded > 150
    # not simply the next power of two: 53 000 samples per code would run on 131 072 points
    assert f(53000) < 131072


def test_length_out_of_range_is_an_argument_error():
    m = pkg()
    for n in (0, 1, -5, 2 ** 29 + 1):
        with pytest.raises(m._native.SgxError):
            m._native.acquire_fft_length(n)


@pytest.mark.parametrize("fs,IF", any_rate.RATES, ids=any_rate.RATE_IDS)
def test_padded_search_is_the_references_search(fs, IF):
    """The premise: at the chooser's length, the padded search in numpy gives oracle.acquire's bin and code phase exactly
    and its peakMetric to 1e-12, for all six PRNs searched."""
    o = any_rate.oracle_settings(fs, IF)
    n = o.samplesPerCode
    assert n == int(round(fs / 1000)) and not any_rate.smooth(n)
    length = pkg()._native.acquire_fft_length(n)
    x = any_rate.record(fs, IF)[:11 * n]
    want = orc.acquire(o, x)
    idx = [p - 1 for p in any_rate.PRNS]
    peaks = spec.acquire(o, x, 1, 2, False, 500.0, prn_indices=idx, details=True)["details"]   # (absent PRNs' peaks too)
    got = any_rate.padded_acquire(o, x, length, idx)
    for p, (fbi, c, metric) in got.items():
        assert fbi == want["freqBin"][p] == peaks[p]["bins"][0][1], p
        assert c == peaks[p]["samples"][0][1], p
        if want["carrFreq"][p] > 0:
            assert c == want["codePhase"][p], p
        assert abs(metric / want["peakMetric"][p] - 1.0) <= 1e-12, (p, metric, want["peakMetric"][p])
    assert [p + 1 for p in range(32) if want["carrFreq"][p] > 0] == [2, 5]


@pytest.mark.parametrize("case", any_rate.search_cases(), ids=[c[0] for c in any_rate.search_cases()])
def test_search_is_well_conditioned(case):
    name, rate, signal, n_blocks, noncoh = case
    o = any_rate.oracle_settings(*any_rate.RATES[rate])
    x = signal()
    w, gap, room = any_rate.conditioned(o, x, n_blocks, noncoh)
    print("\n%s: smallest gap %.2e, closest metric to the threshold %.3f" % (name, gap, room))
    ref = orc.acquire(o, x, n_blocks=n_blocks, noncoh=noncoh)
    for k in ("carrFreq", "codePhase", "freqBin", "fineIdx"):
        assert np.array_equal(w[k], ref[k]), k
    assert gap >= any_rate.GAP, gap
    assert room >= any_rate.THRESHOLD_ROOM, room
    assert [p + 1 for p in range(32) if ref["carrFreq"][p] > 0] == [2, 5]


@pytest.mark.parametrize("c", any_rate.EDGE_PHASES)
def test_edge_scene_puts_the_peak_where_it_is_meant(c):
    """The oracle's peak really lands on code phase c (for c = samples per chip it raises the reference's IndexError, and
    the search grid's arg-max is c), and the scene is as well conditioned as the others."""
    o = any_rate.edge_settings()
    n, spc = any_rate.EDGE_N, any_rate.EDGE_SPC
    assert o.samplesPerCode == n and int(round(o.samplingFreq / o.codeFreqBasis)) == spc
    x = any_rate.edge_record(c)
    res = any_rate.padded_peaks(o, x.astype(np.float64), pkg()._native.acquire_fft_length(n), 0)
    assert int(res.max(0).argmax()) == c
    assert spec.rel_gap(spec._top2(res.max(0))) >= any_rate.GAP and spec.rel_gap(spec._top2(res.max(1))) >= any_rate.GAP
    if c == spc:
        with pytest.raises(IndexError):
            orc.acquire(o, x)
        return
    w = spec.acquire(o, x, 1, 2, False, 500.0, prn_indices=[0], details=True)
    ref = orc.acquire(o, x)
    assert ref["codePhase"][0] == c and ref["carrFreq"][0] > 0 and w["fineIdx"][0] == ref["fineIdx"][0]
    d = w["details"][0]
    assert min(spec.rel_gap(d[k]) for k in ("bins", "samples", "fine")) >= any_rate.GAP
    assert abs(ref["peakMetric"][0] / o.acqThreshold - 1.0) >= any_rate.THRESHOLD_ROOM
    if c == n - 1 - spc:
        assert orc.exclusion_index(c, n, spc)[0] == -1        # the list that starts at -1 and wraps


@pytest.mark.parametrize("name", [c.name for c in any_rate.COHERENT_CASES])
def test_coherent_case_is_well_conditioned(name):
    """The two coherent searches on the padded direct path, by the rules of tests/test_coherent_acq_cases.py; nothing is
    dropped."""
    c = any_rate.COHERENT_BY_NAME[name]
    assert c.g["path"] == "direct" and not c.drop and not c.no_fine and c.g["prn_chunk"] == c.prn_chunk
    assert not any_rate.smooth(c.s.samplesPerCode)
    ref = c.reference()
    rows = {r["prn"]: r for r in c.sats()}
    for p, gaps in conditioning(c, ref).items():
        lo, hi = c.phase_range(rows[p])
        assert ref["peakMetric"][p] >= 1.2 * c.s.acqThreshold and ref["carrFreq"][p] > 0, p
        assert ref["freqBin"][p] == rows[p]["bin"] and lo - 2 <= ref["codePhase"][p] <= hi + 2, p
        assert min(g for g, _ in gaps) >= any_rate.GAP, (p, gaps)
