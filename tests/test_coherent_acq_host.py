"""CPU-only checks of the coherent multi-millisecond acquisition (include/sgx.h, sgx_acquire_coherent): the library's plan
against the numpy contract (tests/coherent_acq_spec.py), the argument checks, the contract against the oracle at 1 ms,
and the Settings / postProcessing surface.  No kernel runs here."""
import importlib

import numpy as np
import pytest

import coherent_acq_spec as spec
import weak_scene
from conftest import pkg
from oracle import softgnss_oracle as orc


@pytest.fixture(scope="module")
def m():
    importlib.import_module("__graft_entry__").build()
    return pkg()


def _rate2(m):
    s = m.Settings()
    s.samplingFreq = 16367600.0
    s.IF = 4130400.0
    return s


@pytest.mark.parametrize("T,M,noncoh,step,band", [
    (1, 2, False, None, 14.0), (5, 4, False, None, 14.0), (10, 10, True, None, 14.0), (10, 10, False, None, 14.0),
    (20, 20, True, None, 14.0), (1, 3, True, 250.0, 14.0),
    (2, 2, False, 15.0, 1.0),        # 68 bins, 68 distinct fractions: the direct path
    (4, 2, True, 11.0, 1.0),
])
def test_plan_matches_spec(m, T, M, noncoh, step, band):
    s = m.Settings()
    s.acqSearchBand = band
    got = m._native.acquire_coherent_plan(s, T, M, noncoh, step)
    want = spec.grid(s, T, M, noncoh, step)
    for k in ("n_bins", "n_phi", "path", "prn_chunk", "bin_runs"):
        assert got[k] == want[k], (k, got, want)


def test_plan_paths(m):
    s = m.Settings()
    p = m._native.acquire_coherent_plan(s, 10, 10, True, None)
    assert (p["n_bins"], p["n_phi"], p["path"]) == (281, 20, "shift")          # 50 Hz over 14 kHz
    assert p["bin_runs"] > 1 and p["prn_chunk"] == 1
    assert m._native.acquire_coherent_plan(s, 20, 2, False, None)["n_bins"] == 561
    s.acqSearchBand = 1.0
    assert m._native.acquire_coherent_plan(s, 2, 2, False, 15.0)["path"] == "direct"
    r2 = m._native.acquire_coherent_plan(_rate2(m), 10, 4, True, None)          # the second front end
    want = spec.grid(_rate2(m), 10, 4, True, None)
    assert r2["path"] == want["path"] == "direct"
    assert (r2["n_bins"], r2["n_phi"]) == (want["n_bins"], want["n_phi"])


@pytest.mark.parametrize("kw", [dict(coherent_ms=0), dict(coherent_ms=21), dict(bin_step_hz=0.0),
                                dict(bin_step_hz=-50.0), dict(bin_step_hz=10.0), dict(n_windows=0),
                                dict(n_windows=65), dict(coherent_ms=20, n_windows=21)])
def test_plan_rejects_bad_arguments(m, kw):
    s = m.Settings()
    args = dict(coherent_ms=10, n_windows=10, noncoh=True, bin_step_hz=None)
    args.update(kw)
    with pytest.raises(m._native.SgxError) as e:
        m._native.acquire_coherent_plan(s, **args)
    assert e.value.code == m._native.SGX_E_ARG
    with pytest.raises(spec.ArgError):
        spec.grid(s, args["coherent_ms"], args["n_windows"], args["noncoh"], args["bin_step_hz"])


def test_plan_rejects_direct_path_overflow(m):
    s = m.Settings()
    s.acqSearchBand = 10.0
    with pytest.raises(m._native.SgxError) as e:      # 668 bins x 4 windows with 200 fractions
        m._native.acquire_coherent_plan(s, 4, 4, False, 15.0)
    assert e.value.code == m._native.SGX_E_ARG and "direct path" in str(e.value)


@pytest.fixture(scope="module")
def small_record():
    sats = ((1, 52.0, 210.0, 5000), (6, 50.0, -380.0, 20000))
    return weak_scene.generate(12, sats=sats, seed=7)


@pytest.mark.parametrize("noncoh,blocks", [(False, 2), (True, 3)])
def test_spec_equals_oracle_at_one_ms(small_record, noncoh, blocks):
    o = orc.OracleSettings(acqSearchBand=2.0)
    x = small_record[:11 * o.samplesPerCode]
    want = orc.acquire(o, x, n_blocks=blocks, noncoh=noncoh, prn_indices=[1, 6, 9])
    got = spec.acquire(o, x, coherent_ms=1, n_windows=blocks, noncoh=noncoh, bin_step_hz=500.0, prn_indices=[1, 6, 9])
    assert got["carrFreq"][1] > 0 and got["carrFreq"][6] > 0
    for k in ("carrFreq", "codePhase", "peakMetric", "freqBin", "fineIdx"):
        assert np.array_equal(got[k], want[k]), k


def test_settings_defaults(m):
    s = m.Settings()
    assert (s.acqCoherentMs, s.acqBlocks, s.acqNonCoherent, s.acqBinStep) == (1, 2, False, None)
    assert s.acquisitionLength() == 11 * s.samplesPerCode
    s.acqCoherentMs, s.acqBlocks = 10, 10
    assert s.acquisitionLength() == 100 * s.samplesPerCode


class _StubAcq(object):
    calls = []

    def __init__(self, settings, *a, **k):
        self.carrFreq = np.zeros(32)

    def acquire(self, data, **kw):
        _StubAcq.calls.append((len(data), kw))


@pytest.mark.parametrize("T,M,noncoh", [(1, 2, False), (10, 10, True), (2, 3, False)])
def test_post_processing_reads_and_passes_the_search(m, monkeypatch, tmp_path, T, M, noncoh):
    s = m.Settings()
    n = s.samplesPerCode
    f = tmp_path / "rec.bin"
    np.zeros(120 * n, dtype=np.int8).tofile(str(f))
    s.acqCoherentMs, s.acqBlocks, s.acqNonCoherent = T, M, noncoh
    monkeypatch.setattr(pkg("acquisition"), "AcquisitionResult", _StubAcq)
    _StubAcq.calls = []
    acq, trk, nav = s.postProcessing(str(f))
    assert trk is None and nav is None
    assert _StubAcq.calls == [(max(11, T * M) * n, dict(n_blocks=M, noncoh=noncoh, coherent_ms=T, bin_step_hz=None))]


def test_sharded_path_refuses_coherent_windows(m):
    with pytest.raises(ValueError, match="coherent_ms"):
        pkg("shard").acquire_sharded(None, None, 0, 1, None, coherent_ms=10)


def test_main_flags(m, monkeypatch):
    seen = {}

    def fake(self, fileNameStr=None):
        seen.update(T=self.acqCoherentMs, M=self.acqBlocks, nc=self.acqNonCoherent)
        return None, None, None
    monkeypatch.setattr(pkg("initialize").Settings, "postProcessing", fake)
    pkg("main").main(["x.bin", "--no-probe", "--acq-coherent-ms", "10", "--acq-blocks", "8", "--acq-noncoh"])
    assert seen == dict(T=10, M=8, nc=True)
