"""The table of tests/silent_cases.py against the oracle alone: every expectation the GPU tests (tests/test_silent_gpu.py) hold
the product to is the reference's own behaviour, the ValueError included.  Needs no GPU.  The host side of the product's
answer - one error code and one exception for a silent channel - is at the end."""
import numpy as np
import pytest

import silent_cases as sc
from conftest import pkg
from oracle import softgnss_oracle as orc

DATA_FAMILIES = [f.name for f in sc.FAMILIES if f.data == f.name]


@pytest.mark.parametrize("name", sc.ALL_NAN)
def test_silent_and_non_finite_searches_give_nan_metrics(name):
    """zeros of every type, and a record with one NaN or +Inf sample in the second block: every metric NaN, freqBin 0, nothing
    detected, every channel off"""
    for path in ("acquire", "f64"):
        r = sc.search_expect(name, path)
        assert np.isnan(r["peakMetric"]).all() and np.all(r["freqBin"] == 0), (name, path)
        assert not r["carrFreq"].any() and not r["codePhase"].any() and np.all(r["fineIdx"] == -1)
        assert not orc.pre_run(sc.oracle_settings(), r)["PRN"].any()


def test_a_non_finite_sample_poisons_every_power_of_its_block():
    """what the product's answer rests on: with one NaN or +Inf sample in a block, every power the reference forms from that
    block (acquisition.py:120-126) is NaN, for every bin"""
    s = sc.oracle_settings()
    n = sc.N
    code_fd = np.fft.fft(orc.make_ca_table(s)[0]).conj()
    for name in ("nan-sample", "inf-sample"):
        x = sc.search_signal(name)
        blk = x[n:2 * n]
        assert np.sum(~np.isfinite(blk)) == 1 and np.isfinite(x[:n]).all()
        ph = np.arange(n) * 2 * np.pi / s.samplingFreq
        with np.errstate(invalid="ignore", over="ignore"):
            for f in orc.freq_bins(s)[[0, 14, 28]]:
                spectrum = np.fft.fft(np.sin(f * ph) * blk + 1j * (np.cos(f * ph) * blk))
                assert np.isnan(abs(np.fft.ifft(spectrum * code_fd)) ** 2).all(), (name, f)


def test_noise_only_stays_clear_of_a_detection_and_of_ties():
    r = sc.search_expect("noise-only")
    top = float(r["peakMetric"].max())
    print("noise-only: largest of the 32 metrics %.4f, acqThreshold %.2f" % (top, sc.oracle_settings().acqThreshold))
    assert top <= 0.9 * sc.oracle_settings().acqThreshold
    assert not r["carrFreq"].any()
    clear = sc.clear_of_a_tie(sc.search_signal("noise-only"))
    print("noise-only: %d of 32 PRNs at least %g clear of a tie between bins" % (clear.sum(), sc.TIE_GAP))
    assert clear.sum() >= 24


@pytest.mark.parametrize("name", sorted(sc.BLOCK_SEL))
def test_one_silent_block_decides_the_block_choice(name):
    r = sc.search_expect(name)
    found = np.flatnonzero(r["carrFreq"] > 0)
    assert found.size >= 6, found
    assert np.all(r["blockSel"][found] == sc.BLOCK_SEL[name]), r["blockSel"][found]
    # ... and the search of the untouched scene chooses both blocks: the rule is not decisive there
    whole = sc.search_expect("scene")
    assert set(np.unique(whole["blockSel"][found])) == {0, 1}


def test_late_signal_has_no_channel_to_track():
    r = sc.search_expect("late-signal")
    assert np.array_equal(sc.late_signal_record()[:sc.SEARCH_MS * sc.N], sc.search_signal("late-signal"))
    assert sc.late_signal_record()[sc.SEARCH_MS * sc.N:].any()
    assert not orc.pre_run(sc.oracle_settings(), r)["PRN"].any()


def test_the_coherent_contract_on_the_same_arrays():
    """2 windows of 2 ms: zeros give NaN; the non-finite sample lies in window 0, so the later window wins and the metrics are
    finite - the contract compared against is whatever the spec gives"""
    z = sc.search_expect("zeros-int8", "coherent")
    prns = list(sc.COHERENT_PRNS)
    assert np.isnan(z["peakMetric"][prns]).all() and np.all(z["freqBin"][prns] == 0)
    nn = sc.search_expect("nan-sample", "coherent")
    assert np.isfinite(nn["peakMetric"][prns]).all()
    assert np.isnan(sc.search_expect("nan-sample", "coherent-noncoh")["peakMetric"][prns]).all()


@pytest.mark.parametrize("family", DATA_FAMILIES)
@pytest.mark.parametrize("case", sorted(sc.TRACKING))
def test_tracking_table_is_the_oracles(case, family):
    exp = sc.track_expect(case, family)
    fam = sc.FAMILY[family]
    assert len(exp) == fam.nch
    ks = [e["k"] for e in exp]
    print("%s / %s: first block of zero sums per channel %r" % (case, family, ks))
    if case == "short-gap":
        assert ks == [None] * fam.nch
        for e in exp:
            assert not e["raises"] and e["rows"].shape == (13, sc.TRACK_MS) and np.isfinite(e["rows"]).all()
        return
    if case == "silent-from-start":
        assert ks == [0] * fam.nch
    else:
        assert ks[0] == sc.GAP_BLOCK + 1                     # block 12 partly silent and finite, block 13 all zero
        # (another channel's blocks lie up to one block earlier or later against channel 0's)
        assert all(sc.GAP_BLOCK <= k <= sc.GAP_BLOCK + 2 for k in ks if k is not None)
    if case != "one-block-gap":
        assert None not in ks
    for e in exp:
        k = e["k"]
        if k is None:                                        # (one-block-gap: no whole block of this channel is silent)
            assert not e["raises"] and np.isfinite(e["rows"]).all()
            continue
        rows = e["rows"]
        assert e["raises"] and rows.shape == (13, k + 1)     # step() of block k + 1 raised ValueError
        assert np.isfinite(rows[:, :k]).all()
        assert np.all(rows[3:9, k] == 0.0) and np.isfinite(rows[0, k])
        assert np.isnan(rows[[1, 2, 9, 10, 11, 12], k]).all()
    # the whole-run entry point dies the same way
    ch = sc.channels(fam.fs, fam.IF, fam.nch)
    phase = sc.start_bytes(fam).astype(np.float64)
    with pytest.raises(ValueError, match="NaN"), np.errstate(divide="ignore", invalid="ignore"):
        orc.track(sc.track_settings(fam), dict(ch, codePhase=phase), sc.track_record(case, family))


def test_uint8_silence_is_byte_zero():
    fam = sc.FAMILY["uint8"]
    lo, hi = sc.silent_span("silent-from-k", fam)
    rec = sc.track_record("silent-from-k", "uint8")
    assert rec.dtype == np.uint8 and not rec[lo:hi].any() and abs(float(rec[:lo].mean()) - 128.0) < 1.0


# ---- the product's host side ---------------------------------------------------------------------------------------------------
def test_a_silent_channel_is_a_value_error_with_its_results():
    nat = pkg("_native")
    assert nat.SGX_E_SILENT == -8 and issubclass(nat.SilentChannelError, ValueError)
    assert not issubclass(nat.SilentChannelError, nat.SgxError)
    e = nat.SilentChannelError("x", np.zeros((1, 13, 2)), np.ones(1, dtype=np.int32))
    assert e.code == nat.SGX_E_SILENT and e.series.shape == (1, 13, 2) and e.ms_done[0] == 1


def test_the_header_names_the_code():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgx.h")).read()
    assert "#define SGX_E_SILENT   -8" in text
