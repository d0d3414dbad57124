"""The excision stage without a GPU: the kernel's work items in a host loop (sgx_excise_host) against the numpy contract of
tests/excise_spec.py on every case of tests/excise_cases.py, the items' spectra against numpy.fft.rfft, sgx_excise_plan
against the contract's segment counts, every refusal, the settings and the command line, and the chirp scene
(tests/chirp_scene.py) through the contract and the oracle's acquisition.  The refusal of a record beyond one launch cannot
be reached: 2^31 tiles are more than 7e12 samples.  Run with -m "not gpu"."""
import ctypes as C
import importlib

import numpy as np
import pytest

import chirp_scene
import excise_cases as cases
import excise_spec as spec
from conftest import pkg

FIGURES = ("segments", "bins_cut", "segments_cut", "clipped")


@pytest.fixture(scope="module")
def built():
    importlib.import_module("__graft_entry__").build()
    return pkg()


@pytest.mark.parametrize("c", cases.CASES, ids=[c.name for c in cases.CASES])
def test_the_host_items_equal_the_contract(built, c):
    y, info = built._native.excise_host(c.x, c.N, c.threshold, c.passes)
    y0, info0 = c.reference()
    assert y.tobytes() == y0.tobytes(), "first difference at sample %d" % int(np.flatnonzero(y != y0)[0])
    assert [info[k] for k in FIGURES] == [info0[k] for k in FIGURES]
    assert np.array_equal(info["cut_per_segment"], info0["cut_per_segment"])


def test_the_items_spectra_are_numpy_s_to_a_hundredth_of_the_margin(built):
    """The largest difference over every segment of every case, relative to the largest bin of its segment length's cases:
    3.7e-16 at N = 64, 5.7e-16 at N = 256, 5.6e-16 at N = 1024 when this was written."""
    worst = {}
    for c in cases.CASES:
        H, n = c.N // 2, c.x.size
        J = spec.segments(n, c.N)
        xp = np.zeros((J + 1) * H)
        xp[H:H + n] = c.x
        want = np.array([np.fft.rfft(xp[j * H:j * H + c.N] * spec.window(c.N)) for j in range(J)])
        got = built._native.excise_host_spectra(c.x, c.N)
        assert got.shape == want.shape
        err = float(np.abs(got - want).max() / np.abs(want).max())
        worst[c.N] = max(worst.get(c.N, 0.0), err)
    print("largest relative difference of the spectra per segment length: %r" % (worst,))
    assert max(worst.values()) <= spec.MARGIN / 100.0      # relative to the largest bin, as the bound in the spec


def test_the_plan_counts_the_contract_s_segments(built):
    n_ = built._native
    for N in (64, 128, 256, 512, 1024):
        H = N // 2
        S = n_.excise_plan(1, N)[1]
        assert S == 8192 // N
        edges = [1, H, N, 7 * H, (S - 1) * H, 3 * (S - 1) * H, 1 << 20, (1 << 32) + 5 * H]
        for n in sorted({max(1, e + d) for e in edges for d in (-1, 0, 1)}):
            assert n_.excise_plan(n, N) == (spec.segments(n, N), S), (n, N)


def test_every_refusal(built):
    n_ = built._native
    x = np.zeros(1000, dtype=np.int8)
    y = np.zeros(1000, dtype=np.int8)
    info = n_.ExciseInfo()

    def host(n=1000, N=256, threshold=8.0, passes=3, xp=x, yp=y, ip=info):
        return n_.lib().sgx_excise_host(None if xp is None else n_._ptr(xp), n, N, threshold, passes,
                                        None if yp is None else n_._ptr(yp), None if ip is None else C.byref(ip), None)

    assert host() == n_.SGX_OK
    for N in (0, -256, 32, 96, 255, 257, 2048, 1 << 30):
        assert host(N=N) == n_.SGX_E_ARG and "power of two in 64 .. 1024" in n_.last_error(), N
        with pytest.raises(ValueError):
            n_.excise_plan(1000, N)
    for t in (0.0, 0.999, -8.0, float("nan"), float("inf"), -float("inf")):
        assert host(threshold=t) == n_.SGX_E_ARG and "threshold" in n_.last_error(), t
    for p in (0, -1, 9, 100):
        assert host(passes=p) == n_.SGX_E_ARG and "passes" in n_.last_error(), p
    assert host(n=0) == n_.SGX_E_ARG and "at least one sample" in n_.last_error()
    with pytest.raises(ValueError):
        n_.excise_plan(0, 256)
    assert host(xp=None) == n_.SGX_E_ARG and host(yp=None) == n_.SGX_E_ARG and host(ip=None) == n_.SGX_E_ARG
    J, S = C.c_int64(0), C.c_int32(0)
    assert n_.lib().sgx_excise_plan(1000, 256, None, C.byref(S)) == n_.SGX_E_ARG
    assert n_.lib().sgx_excise_plan(1000, 256, C.byref(J), None) == n_.SGX_E_ARG
    assert n_.lib().sgx_excise_timing(None, None) == n_.SGX_E_ARG
    assert n_.lib().sgx_if_excise(None, None, 256, 8.0, 3, None, None, None) == n_.SGX_E_ARG
    assert n_.lib().sgx_excise_host_spectra(n_._ptr(x), 1000, 256, None) == n_.SGX_E_ARG
    assert not y.any()                                   # a refused call writes nothing


def test_the_settings_and_the_options_reach_settings(built, monkeypatch, capsys):
    s = built.Settings()
    assert (s.sweptMitigation, s.exciseSegment, s.exciseThreshold, s.excisePasses) == (False, 256, 8.0, 3)
    main = pkg("main")
    seen = {}
    monkeypatch.setattr(built.Settings, "postProcessing",
                        lambda self, fileNameStr=None: seen.update(vars(self)) or (None, None, None))
    look = ("sweptMitigation", "exciseSegment", "exciseThreshold", "excisePasses", "interferenceMitigation")
    for argv, want in ((["x.bin", "--no-probe"], (False, 256, 8.0, 3, False)),
                       (["x.bin", "--no-probe", "--excise"], (True, 256, 8.0, 3, False)),
                       (["x.bin", "--no-probe", "--excise=5.5", "--excise-segment", "128"], (True, 128, 5.5, 3, False)),
                       (["x.bin", "--no-probe", "--excise", "--notch"], (True, 256, 8.0, 3, True))):
        seen.clear()
        assert main.main(argv) == 0
        assert tuple(seen[k] for k in look) == want, argv
    for argv in (["x.bin", "--excise-segment", "128"], ["x.bin", "--excise=0.5"], ["x.bin", "--excise", "--excise-segment", "96"],
                 ["x.bin", "--excise", "--excise-segment", "2048"]):
        with pytest.raises(SystemExit):
            main.main(argv)
    capsys.readouterr()
    for option in ("--excise", "--excise-segment"):
        assert option in main.__doc__


def test_excise_reads_int8_records_only(built):
    s = built.Settings()
    s.dataType = "int16"
    with pytest.raises(ValueError, match="int8 records only"):
        s.excise(None)


def test_the_chirp_takes_the_satellites_and_the_excision_brings_them_back():
    clean, raw, exc = (chirp_scene.search(k) for k in ("clean", "raw", "excised"))
    p = chirp_scene.PRN_INDICES
    found = [int(np.count_nonzero(r["carrFreq"][p])) for r in (clean, raw, exc)]
    info = chirp_scene.excised()[1]
    print("found: clean %d, raw %d, excised %d; metrics raw <= %.2f, excised >= %.2f; cells cut %.4f, clipped %d"
          % (found[0], found[1], found[2], raw["peakMetric"][p].max(), exc["peakMetric"][p].min(),
             info["bins_cut"] / float(info["segments"] * 127), info["clipped"]))
    x = chirp_scene.record()
    assert x.size == 12 * chirp_scene.settings().samplesPerCode and np.abs(x.astype(int)).max() < 127
    assert found[0] == len(p)
    assert found[1] <= found[0] // 2
    assert found[2] == found[0]
    assert np.array_equal(exc["codePhase"][p], clean["codePhase"][p])
    assert np.array_equal(exc["freqBin"][p], clean["freqBin"][p])
