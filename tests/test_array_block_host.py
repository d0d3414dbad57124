"""CPU-only checks of the block-adaptive antenna combiner (include/sgx.h: sgx_array_design_blocks, and what of
sgx_array_block_stats, sgx_if_combine_blocks and the stage needs no record) against the numpy contract of
tests/array_block_spec.py: the design of every block to the bit, its equivalence to sgx_array_design, the window sums, the
hold rule, every refusal that needs no GPU, the Settings and command-line surface, the moving-jammer scene of
tests/array_block_cases.py shown to be what it claims by the contracts plus the oracle alone, the host cost of the design,
and a stand-alone program under AddressSanitizer and UBSan.  Run with -m "not gpu"."""
import ctypes as C
import importlib
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import array_block_cases as bcases
import array_block_spec as bspec
import array_spec as spec
from conftest import pkg
from test_array_host import SHAPES, correlated_record

B = bspec.BLOCK_UNIT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = [(W, nb) for W in (1, 3, 5) for nb in (1, 2, 5)]


@pytest.fixture(scope="module")
def built():
    importlib.import_module("__graft_entry__").build()
    return pkg()


def block_record(rng, n_blocks, lanes, A, last=333):
    """Correlated streams over n_blocks blocks, the last one `last` frames short of nothing: F = (n_blocks - 1) B + last."""
    return correlated_record(rng, (n_blocks - 1) * B + last, lanes, A)


def same_blocks(n, rho, F, Bf, W, lanes, ref=0, loading=spec.DEFAULT_LOADING, target=spec.DEFAULT_TARGET_RMS):
    want = bspec.design_blocks(rho, F, Bf, W, lanes, ref, loading, target)
    taps, shift, info = n.array_design_blocks(rho, F, Bf, W, lanes, ref, loading, target)
    what = (rho.shape, F, Bf, W, ref)
    assert taps.dtype == np.int16 and taps.shape == want[0].shape and np.array_equal(taps, want[0]), what
    assert shift == want[1] == n.ARRAY_SHIFT
    assert np.array_equal(info["gain"], want[2]) and np.array_equal(info["suppression_db"], want[3]), what     # exactly
    assert np.array_equal(info["weights"], want[4]) and np.array_equal(info["status"], want[5]), what
    bspec.check_blocks(taps, shift, Bf, lanes, rho.shape[1], 0, F * rho.shape[1] * lanes)    # what it designs, the combiner takes
    return want


# ---- the design function ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("A,K", SHAPES)
def test_block_design_equals_the_contract(built, lanes, A, K):
    """Every (A, K) and both kinds; the windows and block counts in turn, all nine pairs at the smallest shape."""
    n = built._native
    turn = 2 * SHAPES.index((A, K)) + lanes
    plans = PLANS if (A, K) == SHAPES[0] else [PLANS[turn % 9], PLANS[(turn + 4) % 9]]
    if (A, K) == SHAPES[-1]:                     # (the turns alone reach every pair of window and block count as well)
        assert set(PLANS[(2 * i + la + d) % 9] for i in range(1, len(SHAPES)) for la in (1, 2) for d in (0, 4)) == set(PLANS)
    rng = np.random.default_rng(300 * A + 10 * K + lanes)
    rhos = {}
    for W, nb in plans:
        if nb not in rhos:
            b = block_record(rng, nb, lanes, A)
            rhos[nb] = bspec.block_stats(b, lanes, A, K, B)
            assert np.array_equal(rhos[nb].sum(axis=0), spec.stats(b, lanes, A, K))           # by construction
        F = (nb - 1) * B + 333
        want = same_blocks(n, rhos[nb], F, B, W, lanes, ref=(W + nb) % A, loading=(1e-3, 0.05)[nb % 2])
        assert not want[5].any() and np.all(want[3] >= -1e-9)
    # a block twice as long, two of them: the same statistics read as blocks of 2 B
    b = correlated_record(rng, 2 * B + 100, lanes, A)
    same_blocks(n, bspec.block_stats(b, lanes, A, K, 2 * B), 2 * B + 100, 2 * B, 3, lanes)


@pytest.mark.parametrize("lanes", [1, 2])
def test_one_block_is_the_existing_design(built, lanes):
    n = built._native
    rng = np.random.default_rng(40 + lanes)
    for A, K in ((2, 1), (4, 5), (8, 7), (3, 15)):
        F = 3000
        b = correlated_record(rng, F, lanes, A)
        rho = spec.stats(b, lanes, A, K)
        assert np.array_equal(bspec.block_stats(b, lanes, A, K, B)[0], rho)
        for ref, loading, target in ((0, 1e-3, 12.0), (A - 1, 0.0, 5.5)):
            t0, s0, i0 = n.array_design(rho, F, lanes, ref, loading, target)
            t1, s1, i1 = n.array_design_blocks(rho[None], F, B, 1, lanes, ref, loading, target)
            assert t1.shape == (1,) + t0.shape and np.array_equal(t1[0], t0) and s1 == s0
            assert i1["gain"][0] == i0["gain"] and i1["suppression_db"][0] == i0["suppression_db"]
            assert np.array_equal(i1["weights"][0], i0["weights"]) and not i1["status"].any()


@pytest.mark.parametrize("lanes", [1, 2])
def test_a_wide_window_gives_every_block_the_whole_record_design(built, lanes):
    n = built._native
    rng = np.random.default_rng(50 + lanes)
    A, K = 4, 3
    for nb in (1, 2, 5, 31):
        F = (nb - 1) * B + 1000
        if nb == 31:                             # (statistics of blocks that differ, without a record of 31 blocks)
            base = bspec.block_stats(block_record(rng, 5, lanes, A), lanes, A, K, B)
            rho = np.stack([base[j % 4] + base[(j // 4) % 4] for j in range(nb)])
        else:
            rho = bspec.block_stats(block_record(rng, nb, lanes, A, 1000), lanes, A, K, B)
        W = 2 * nb + 1 if nb < 31 else 63
        assert W >= 2 * nb
        t0, s0, i0 = n.array_design(rho.sum(axis=0), F, lanes)
        t1, s1, i1 = n.array_design_blocks(rho, F, B, W, lanes)
        for j in range(nb):
            assert np.array_equal(t1[j], t0) and i1["gain"][j] == i0["gain"] and np.array_equal(i1["weights"][j], i0["weights"])
            assert i1["suppression_db"][j] == i0["suppression_db"]
        if nb > 1:                               # ... and a narrow one does not
            assert not np.array_equal(n.array_design_blocks(rho, F, B, 1, lanes)[0][0], t0)


@pytest.mark.parametrize("lanes", [1, 2])
def test_the_hold_rule(built, lanes):
    n = built._native
    rng = np.random.default_rng(60 + lanes)
    A, K, nb = 3, 3, 7
    F = (nb - 1) * B + 333
    full = bspec.block_stats(block_record(rng, nb, lanes, A), lanes, A, K, B)
    # a zero stretch of two blocks in the middle
    rho = full.copy()
    rho[3:5] = 0
    want = same_blocks(n, rho, F, B, 1, lanes)
    assert list(want[5]) == [0, 0, 0, 1, 1, 0, 0]
    for j in (3, 4):
        assert np.array_equal(want[0][j], want[0][2]) and want[2][j] == want[2][2] and want[3][j] == want[3][2]
    assert not np.array_equal(want[0][5], want[0][2])
    assert not same_blocks(n, rho, F, B, 3, lanes)[5].any()                    # every window of three reaches a live block
    # one at the start: it takes the block behind it; with two more zero blocks the window of three holds too
    rho = full.copy()
    rho[0] = 0
    want = same_blocks(n, rho, F, B, 1, lanes)
    assert list(want[5]) == [1, 0, 0, 0, 0, 0, 0] and np.array_equal(want[0][0], want[0][1]) and want[2][0] == want[2][1]
    rho[1:3] = 0
    want = same_blocks(n, rho, F, B, 3, lanes)
    assert list(want[5]) == [1, 1, 0, 0, 0, 0, 0] and np.array_equal(want[0][0], want[0][2])
    assert np.array_equal(want[0][1], want[0][2]) and np.array_equal(want[4][0], want[4][2])
    # the last block
    rho = full.copy()
    rho[6] = 0
    assert list(same_blocks(n, rho, F, B, 1, lanes)[5]) == [0, 0, 0, 0, 0, 0, 1]
    # an all-zero record: refused with the text sgx_array_design gives
    zero = np.zeros_like(full)
    with pytest.raises(n.SgxError) as today:
        n.array_design(zero[0], B, lanes)
    for W in (1, 3):
        with pytest.raises(n.SgxError) as e:
            n.array_design_blocks(zero, F, B, W, lanes)
        assert str(e.value) == str(today.value) and "positive definite" in str(e.value) and "all-zero record" in str(e.value)
        with pytest.raises(ValueError, match="positive definite"):
            bspec.design_blocks(zero, F, B, W, lanes)
    # the optional outputs may be left out
    taps = np.zeros((nb, A, K, lanes), dtype=np.int16)
    shift = C.c_int32(0)
    assert n.lib().sgx_array_design_blocks(n._ptr(full), nb, F, B, 3, lanes, A, K, 0, 1e-3, 12.0, n._ptr(taps), C.byref(shift),
                                           None, None, None, None) == n.SGX_OK
    assert np.array_equal(taps.reshape(want[0].shape), bspec.design_blocks(full, F, B, 3, lanes)[0])


# ---- refusals -----------------------------------------------------------------------------------------------------------

def test_design_refusals(built):
    n = built._native
    rng = np.random.default_rng(8)
    A, K, nb = 4, 3, 3
    F = 2 * B + 500
    rho = bspec.block_stats(block_record(rng, nb, 1, A, 500), 1, A, K, B)
    big = np.zeros(4 * 8 * 8 * 15 * 2, dtype=np.int64)                         # room for every shape that is refused
    big[:rho.size] = rho.ravel()
    taps, w = np.zeros(4 * 256, dtype=np.int16), np.zeros(4 * 256)
    gain, supp, status, shift = np.zeros(4), np.zeros(4), np.zeros(4, dtype=np.uint8), C.c_int32(0)

    def rc(rho_=big, nb_=nb, F_=F, B_=B, W=3, lanes=1, A_=A, K_=K, ref=0, loading=1e-3, target=12.0, null=None):
        ptrs = dict(rho=n._ptr(rho_), taps=n._ptr(taps), shift=C.byref(shift))
        if null:
            ptrs[null] = None
        return n.lib().sgx_array_design_blocks(ptrs["rho"], nb_, F_, B_, W, lanes, A_, K_, ref, loading, target, ptrs["taps"],
                                               ptrs["shift"], n._ptr(w), n._ptr(gain), n._ptr(supp), n._ptr(status))

    def refused(word, **kw):
        assert rc(**kw) == n.SGX_E_ARG and word in n.last_error(), (kw, n.last_error())

    assert rc() == n.SGX_OK
    for name in ("rho", "taps", "shift"):
        refused(name, null=name)
    for lanes in (0, 3):
        refused("lanes", lanes=lanes)
    for A_ in (1, 9):
        refused("A =", A_=A_)
    for K_ in (0, 2, 17):
        refused("K =", K_=K_)
    refused("A K", A_=8, K_=9)
    for ref in (-1, 4):
        refused("ref", ref=ref)
    for loading in (-1e-3, np.inf, np.nan):
        refused("loading", loading=loading)
    for target in (0.0, -1.0, 127.5, np.nan):
        refused("target_rms", target=target)
    for B_ in (0, -B, B - 1, B + 1, 2048, 6144):
        refused("B =", B_=B_)
        with pytest.raises(ValueError):
            bspec.blocks_of(F, B_)
    for W in (0, -1, 2, 4, 64, 65):
        refused("W =", W=W)
        with pytest.raises(ValueError):
            bspec.design_blocks(rho, F, B, W, 1)
    for F_ in (0, -5):
        refused("F =", F_=F_)
    for nb_, F_ in ((0, F), (2, F), (4, F), (3, 2 * B), (3, 3 * B + 1), (n.ARRAY_MAX_BLOCKS + 1, (n.ARRAY_MAX_BLOCKS + 1) * B)):
        refused("n_blocks", nb_=nb_, F_=F_)
    with pytest.raises(ValueError):
        bspec.design_blocks(rho, 2 * B, B, 3, 1)
    # a quiet block among live ones at a high target: its reference tap leaves +-32512, and the text names the block
    quiet = rho.copy()
    quiet[1] = bspec.block_stats(rng.integers(-1, 2, B * A).astype(np.int8), 1, A, K, B)[0]
    with pytest.raises(n.SgxError, match="block 1: tap .*32512"):
        n.array_design_blocks(quiet, F, B, 1, 1)
    with pytest.raises(ValueError, match="block 1: a tap"):
        bspec.design_blocks(quiet, F, B, 1, 1)
    n.array_design_blocks(quiet, F, B, 3, 1)                                   # (its neighbours carry the window of three)
    with pytest.raises(ValueError, match="shape"):
        n.array_design_blocks(rho[0], F, B, 3, 1)
    with pytest.raises(ValueError, match="shape"):
        n.array_design_blocks(rho, F, B, 3, 2)


def test_refusals_of_the_device_calls_that_need_no_device(built):
    """What sgx_array_block_stats and sgx_if_combine_blocks refuse before they look at the context or the record."""
    n = built._native
    f, g = n.lib().sgx_if_combine_blocks, n.lib().sgx_array_block_stats
    out, cnt = C.c_void_p(), C.c_int64(-1)
    rho = np.zeros(16, dtype=np.int64)
    good = np.tile(np.arange(-6, 6, dtype=np.int16), 3)                        # 3 blocks x 4 antennas x 3 taps
    wide = np.zeros(3 * 8 * 17 * 2, dtype=np.int16)

    def refused(word, both=True, lanes=1, A=4, taps=good, nb=3, B_=B, K=3, shift=12, flags=0):
        rc = f(None, None, lanes, A, None if taps is None else n._ptr(taps), nb, B_, K, shift, flags, C.byref(out), C.byref(cnt))
        assert rc == n.SGX_E_ARG and word in n.last_error(), (word, rc, n.last_error())
        assert not out.value
        if both:
            rc = g(None, None, lanes, A, K, flags, B_, n._ptr(rho))
            assert rc == n.SGX_E_ARG and word in n.last_error(), (word, rc, n.last_error())

    for lanes in (0, 3):
        refused("lanes", lanes=lanes, taps=wide)
    for A in (0, 1, 9):
        refused("A =", A=A, taps=wide)
    for K in (0, 2, 16, 17):
        refused("K =", K=K, taps=wide)
    refused("A K", A=8, K=9, taps=wide)
    refused("flags", flags=2)
    for B_ in (0, -B, B - 1, B + 16, 2048):
        refused("B =", B_=B_)
    for S in (-1, 31):
        refused("shift", both=False, shift=S)
    refused("taps", both=False, taps=None)
    for nb in (-1, n.ARRAY_MAX_BLOCKS + 1):
        refused("n_blocks", both=False, nb=nb, taps=wide)
    # a tap beyond the bound in block 2 only: the text names the block
    bad = good.copy()
    bad[2 * 12 + 5] = 32513
    refused("block 2", both=False, taps=bad)
    assert "32512" in n.last_error()
    bad = np.tile(np.array([0, 100], dtype=np.int16), 18)
    bad[12 + 3] = -32513
    refused("block 1", both=False, lanes=2, A=2, taps=bad)
    # in bound everywhere: the next refusal is the context's
    refused("c &&", both=True)


# ---- Settings and the command line --------------------------------------------------------------------------------------

def test_settings_defaults_and_block_length(built):
    f = pkg("frontend")
    st = dict((s.name, s) for s in f.STAGES)["combine"]
    assert dict(st.defaults)["arrayBlockMs"] == 0 and dict(st.defaults)["arrayWindowBlocks"] == 3
    s = built.Settings()
    assert (s.arrayBlockMs, s.arrayWindowBlocks) == (0, 3)
    s.antennas = 4
    assert s._array_block_format() is None and s._array_format() == (1, 4, 5, 0, False)
    n = built._native
    assert (n.ARRAY_BLOCK_UNIT, n.ARRAY_MAX_BLOCKS, n.ARRAY_MAX_WINDOW) == (bspec.BLOCK_UNIT, bspec.MAX_BLOCKS, bspec.MAX_WINDOW)
    # B = max(1, round(ms fs / 1000 / 4096)) 4096
    for fs, ms, want in ((4092000.0, 1.0, 4096), (4092000.0, 0.01, 4096), (4092000.0, 10.0, 10 * 4096), (16368000.0, 1.0, 4 * 4096),
                         (16368000.0, 0.4, 2 * 4096), (38192000.0, 2.5, 23 * 4096)):
        s.samplingFreq, s.arrayBlockMs = fs, ms
        assert s._array_block_format() == (want, 3), (fs, ms)
        assert want == max(1, int(round(ms * fs / 1000.0 / 4096))) * 4096
    s.arrayWindowBlocks = 63
    assert s._array_block_format()[1] == 63
    # the walk is the whole-record stage's: positions do not change
    scene = bcases.SCENE.settings(built, arrayBlockMs=1.0, skipNumberOfBytes=8 * bcases.SKIP_FRAMES)
    assert scene._array_block_format() == (bcases.BLOCK_FRAMES, bcases.WINDOW) == (4096, 3)
    assert [(st_.name, a, b) for st_, _, a, b in scene._walk()[0]] == [("combine", 8, 2), ("convert", 2, 2)]
    assert scene._prepared_settings().skipNumberOfBytes == 2 * bcases.SKIP_FRAMES


def test_settings_refusals(built):
    def refused(word, **kw):
        s = built.Settings()
        s.antennas = 4
        for k, v in kw.items():
            setattr(s, k, v)
        with pytest.raises(ValueError, match=word):
            s._array_format()
        with pytest.raises(ValueError, match=word):
            s._walk()

    for v in (-1.0, -1e-9, np.inf, -np.inf, np.nan, "x", None):
        refused("Settings.arrayBlockMs", arrayBlockMs=v)
    for v in (0, 2, 4, 64, 65, -1, 2.5, "x", None):
        refused("Settings.arrayWindowBlocks", arrayBlockMs=1.0, arrayWindowBlocks=v)
    refused("Settings.arrayWindowBlocks", arrayWindowBlocks=2)                 # (refused with the block path off as well)


def test_options(built, monkeypatch, capsys):
    main = pkg("main")
    seen = {}

    def fake_post(self, fileNameStr=None):
        seen.clear()
        seen.update(A=self.antennas, ms=self.arrayBlockMs, W=self.arrayWindowBlocks, K=self.arrayTaps)
        return None, None, None

    monkeypatch.setattr(built.Settings, "postProcessing", fake_post)
    base = ["x.bin", "--no-probe", "--iq", "--fs", "4092000", "--IF", "0", "--antennas", "4"]
    assert main.main(base) == 0 and seen == dict(A=4, ms=0, W=3, K=0)
    assert main.main(base + ["--array-block", "1"]) == 0 and seen == dict(A=4, ms=1.0, W=3, K=0)
    assert main.main(base + ["--array-block", "2.5:5", "--array-taps", "3"]) == 0 and seen == dict(A=4, ms=2.5, W=5, K=3)
    assert main.main(base + ["--array-block", "10:1"]) == 0 and seen == dict(A=4, ms=10.0, W=1, K=0)
    assert "Traceback" not in capsys.readouterr().err
    assert "--array-block" in main.__doc__


REFUSED = [
    ["x.bin", "--array-block", "1"], ["x.bin", "--antennas", "4", "--array-block", "0"],
    ["x.bin", "--antennas", "4", "--array-block", "-1"], ["x.bin", "--antennas", "4", "--array-block", "x"],
    ["x.bin", "--antennas", "4", "--array-block", "inf"], ["x.bin", "--antennas", "4", "--array-block", "nan"],
    ["x.bin", "--antennas", "4", "--array-block", "1:2"], ["x.bin", "--antennas", "4", "--array-block", "1:0"],
    ["x.bin", "--antennas", "4", "--array-block", "1:65"], ["x.bin", "--antennas", "4", "--array-block", "1:x"],
    ["x.bin", "--antennas", "4", "--array-block", "1:3:5"], ["x.bin", "--antennas", "4", "--array-block", ":3"],
]


@pytest.mark.parametrize("argv", REFUSED, ids=[" ".join(a[1:]) for a in REFUSED])
def test_refused_as_a_usage_error(built, monkeypatch, capsys, argv):
    def never(self, *args, **kw):
        raise AssertionError("the run went on")

    for method in ("postProcessing", "probeData", "_prepared_record"):
        monkeypatch.setattr(built.Settings, method, never)
    with pytest.raises(SystemExit) as e:
        pkg("main").main(argv)
    assert e.value.code == 2
    captured = capsys.readouterr()
    message = captured.err.split(": error: ", 1)[1]
    assert any(w in message for w in ("--array-block", "Settings.arrayBlockMs", "Settings.arrayWindowBlocks")), message
    assert "Welcome" not in captured.out and "Traceback" not in captured.err


# ---- the scene: the oracle alone ----------------------------------------------------------------------------------------

def test_the_scene_is_what_it_claims(built):
    """One set of weights for the whole moving-jammer record loses a satellite in every window; a set per millisecond finds
    all four well above the threshold in every window, no other PRN comes near it, no satellite fades under the moving
    null, and every block of the output sits at the target without a clipped sample."""
    scene = bcases.SCENE
    F, Bf = bcases.FRAMES, bcases.BLOCK_FRAMES
    assert abs(2.0 * np.pi * bcases.RATE_HZ * 3 * bcases.RECORD_MS * 1e-3 - 1.9) < 0.05      # antenna 3 moves 1.9 rad
    whole = bcases.combined_whole(scene, F)
    blocks = bcases.combined_blocks(scene, F)
    nb = -(-F // Bf)
    assert blocks["taps"].shape == (nb, 4, 1, 2) and nb == 124 and not blocks["status"].any()
    want = same_blocks(built._native, blocks["rho"], F, Bf, bcases.WINDOW, scene.lanes)      # the library designs these weights
    assert np.array_equal(want[0], blocks["taps"]) and np.array_equal(want[3], blocks["suppression_db"])
    present = np.array(scene.prns) - 1
    absent = np.setdiff1d(np.arange(32), present)
    threshold = scene.oracle_settings().acqThreshold
    print("suppression: whole record %.2f dB, blocks %.2f dB at the least, %.2f dB in the median"
          % (whole["suppression_db"], blocks["suppression_db"].min(), np.median(blocks["suppression_db"])))
    assert whole["suppression_db"] < 15.0 and blocks["suppression_db"].min() > 16.0
    for ms in bcases.WINDOWS_MS:
        assert (ms + 11) * scene.frames_per_ms <= F
        aw = bcases.acquisition(scene, whole["prepared"], ms)
        ab = bcases.acquisition(scene, blocks["prepared"], ms)
        print("window at %d ms: whole record %s, blocks %s, absent at most %.2f"
              % (ms, np.round(aw["peakMetric"][present], 2), np.round(ab["peakMetric"][present], 2), ab["peakMetric"][absent].max()))
        assert np.any(aw["peakMetric"][present] < threshold), (ms, aw["peakMetric"][present])
        assert np.all(ab["peakMetric"][present] >= bcases.MARGIN * threshold), (ms, ab["peakMetric"][present])
        assert np.all(ab["peakMetric"][absent] <= bcases.ABSENT_MAX), (ms, ab["peakMetric"][absent].max())
        assert sorted(np.flatnonzero(ab["carrFreq"]) + 1) == sorted(scene.prns)
    # the oracle tracks the four channels on the block-combined record: no 20 ms stretch behind the pull-in fades
    ref, chans, series = bcases.tracked(scene, blocks["prepared"])
    assert sorted(int(p) for p in chans["PRN"] if p) == sorted(scene.prns) and series.shape[2] == bcases.TRK_MS
    for ch in range(len(scene.prns)):
        stretches = np.array([np.mean(np.abs(series[ch, 3, k:k + 20])) for k in range(40, bcases.TRK_MS, 20)])
        print("PRN %d: mean |I_P| per 20 ms %s" % (chans["PRN"][ch], np.round(stretches)))
        assert stretches.size == 3 and np.all(stretches >= 0.5 * np.median(stretches)), (ch, stretches)
    # every block of the output at the target, nothing clipped
    y = blocks["combined"].astype(np.float64).reshape(-1, 2)
    rms = np.array([np.sqrt(np.mean(y[j * Bf:(j + 1) * Bf] ** 2)) for j in range(nb)])
    print("output rms per block %.3f .. %.3f" % (rms.min(), rms.max()))
    assert np.all(np.abs(rms - spec.DEFAULT_TARGET_RMS) <= bcases.RMS_TOL * spec.DEFAULT_TARGET_RMS), (rms.min(), rms.max())
    assert blocks["clipped"] == 0 and whole["clipped"] == 0


# ---- the host cost of the design, and the design under sanitizers ----------------------------------------------------------

def test_host_cost_of_the_design(built):
    """3 700 blocks - a 37 s record in 10 ms blocks - at three sizes of the system; the times are printed (DESIGN.md section
    4.21 records them), there is no bar on them."""
    n = built._native
    rng = np.random.default_rng(70)
    nb = 3700
    for A, K, lanes in ((4, 5, 1), (8, 1, 2), (8, 7, 2)):
        base = bspec.block_stats(block_record(rng, 4, lanes, A, B), lanes, A, K, B)
        rho = np.ascontiguousarray(base[np.arange(nb) % 4])
        t = time.perf_counter()
        taps, shift, info = n.array_design_blocks(rho, nb * B, B, 3, lanes)
        dt = time.perf_counter() - t
        print("design of %d blocks at A = %d, K = %d, lanes = %d: %.1f ms" % (nb, A, K, lanes, 1e3 * dt))
        assert taps.shape[0] == nb and not info["status"].any()
        assert np.array_equal(taps[5], taps[9]) and np.array_equal(taps[6], taps[10])        # the statistics repeat every four


def test_design_under_sanitizers(tmp_path):
    """tools/array_design_check.cpp, a program of its own, built with AddressSanitizer and UBSan next to the host file
    that holds the design, and run on the CPU: every block's outputs are sized to the byte, a held block included."""
    cxx = shutil.which("g++")
    assert cxx, "no g++ for the host build"
    exe = str(tmp_path / "array_design_check")
    csrc = os.path.join(ROOT, "softgnss-python_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tools", "array_design_check.cpp"), os.path.join(csrc, "sgx_array.cpp"),
                    os.path.join(csrc, "sgx_core.cpp"), "-o", exe, "-lm"], check=True)
    # (the runtimes are linked into the program: it needs nothing preloaded)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "no report" in text and "held blocks" in text, text
