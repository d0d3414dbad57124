"""Strong-signal cancellation without a GPU: the host twin sgx_cancel_host against the numpy contract (tests/cancel_spec.py)
on every case of tests/cancel_cases.py, sgx_cancel_design against design(), every refused argument, and the near-far scene's
claims with the oracle's search and tracking (tests/nearfar_scene.py).  CPU only.

The comparison rule (cancel_cases.compare): the bytes are equal at every sample whose v lies farther than 1e-6 from a
half-integer and differ by at most 1 at the others, which are at most 1e-4 of a case's samples and never within 1e-6 of
+-127.5 - so the clip counts are compared exactly."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cancel_cases as cases
import cancel_spec as spec
import nearfar_scene as nf
from conftest import ROOT, pkg

NEW_SYMBOLS = ("sgx_cancel_design", "sgx_cancel_host", "sgx_cancel_timing", "sgx_if_cancel")


def test_symbols_are_declared_bound_and_exported():
    n = pkg("_native")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sgx_[a-z0-9_]+)\s*\(", text))
    lib = n.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and s in n.SYMBOLS and hasattr(lib, s), s


def test_the_table_covers_what_it_says():
    """The properties the case table is there for, read off the cases themselves."""
    tile = cases.TILE
    per_tile, on_tile, first_on_tile = 0, False, False
    for name in cases.NAMES:
        c = cases.get(name)
        assert 4 <= c["series"].shape[2] <= 40, name
        for st in c["states"]:
            if st is None:
                continue
            done = int(np.count_nonzero(st["blk"]))
            starts = st["start"][:done] - c["off"]
            if done:
                per_tile = max(per_tile, int(np.max(np.bincount(starts // tile))))
                on_tile |= bool(np.any(starts[1:] % tile == 0))
                first_on_tile |= starts[0] % tile == 0
    assert per_tile >= 3 and on_tile and first_on_tile
    assert len(cases.get("one_short")["x"]) < tile and len(cases.get("one_short")["chans"]) == 1
    assert len(cases.get("rate38")["chans"]) == 8 and cases.get("rate38")["s"].samplingFreq == 38.192e6
    assert cases.get("on_tile")["off"] > 0 or cases.get("from_start")["off"] > 0
    off = cases.get("off_done")
    assert [ch[0] for ch in off["chans"]].count(0) == 1 and 0 in off["ms_done"] and 0 < off["ms_done"][3] < 8
    want, v, clipped, covered = cases.expected("off_done")
    assert np.all(want[~covered] == off["x"][~covered]) and np.count_nonzero(want[~covered] == -128) == 3
    assert np.count_nonzero(off["x"][covered] == -128) == 4 and not np.any(want[covered] == -128) and clipped >= 1
    assert cases.expected("clip")[2] > 1000
    assert np.array_equal(cases.expected("nearfar")[0], nf.oracle_cancelled()[1])
    # the hand-made cases
    lane = cases.LANE
    for name, n_ch in (("ch32", 32), ("ch31", 31)):
        c = cases.get(name)
        cover = np.zeros(len(c["x"]), dtype=np.int32)
        for st in c["states"]:
            cover[st["start"][0]:st["start"][-1] + st["blk"][-1]] += 1
        assert len(c["chans"]) == n_ch and [ch[0] for ch in c["chans"]] == list(range(1, n_ch + 1)), name
        assert cover.max() == n_ch and c["series"].shape[2] == 4 and c["s"].samplingFreq == 2.046e6, name
    assert cases.get("ch32")["series"][:31].tobytes() == cases.get("ch31")["series"].tobytes()
    c = cases.get("short_blocks")
    st = c["states"][0]
    first, last = st["start"][1:], st["start"][1:] + st["blk"][1:] - 1
    assert st["blk"][0] >= 2045 and 5 <= st["blk"][1:].min() and st["blk"][1:].max() <= 15
    assert int(np.count_nonzero(first // lane == last // lane)) >= 20
    assert first[0] < cases.TILE < last[-1] and st["rem_code"].max() > 100.0
    other = c["states"][1]
    assert other["start"][0] < first[0] and last[-1] < other["start"][2] + other["blk"][2] and c["ms_done"][1] == 3
    c = cases.get("residues")
    s0, s1 = c["states"]
    assert set((s0["start"][1:] % lane).tolist()) == set(range(lane))        # 0: block k - 1 ends on a lane's last sample
    assert set(s0["blk"].tolist()) == {2045, 2046, 2047}
    inside = [set((st["start"][st["start"] % lane != 0] // lane).tolist()) for st in (s0, s1)]
    assert inside[0] & inside[1]                                              # one lane, a boundary of either channel in it
    ends = max(int(st["start"][-1] + st["blk"][-1]) for st in (s0, s1))
    assert len(c["x"]) == ends - c["off"] and len(c["x"]) % lane != 0
    c = cases.get("far_offset")
    assert c["off"] > 2 ** 33 and len(c["x"]) == 3 * tile - 7
    near = spec.states(c["s"], len(c["x"]), *c["near"], None)
    for far, st in zip(c["states"], near):
        assert np.all(far["start"] > 2 ** 33) and np.array_equal(far["start"] - 2 ** 33, st["start"])
        for f in ("blk", "rem_code", "rem_carr", "step", "carr_freq"):
            assert far[f].tobytes() == st[f].tobytes(), f
    for name in ("ch32", "ch31", "short_blocks", "residues"):                 # amplitudes that are no integers
        assert not np.any(cases.get(name)["amp"] == np.rint(cases.get(name)["amp"])), name
        assert np.abs(cases.get(name)["x"].astype(np.int16)).max() <= 60, name


@pytest.mark.parametrize("name", cases.NAMES)
def test_host_twin_equals_the_contract(name, capsys):
    n = pkg("_native")
    c = cases.get(name)
    y, clipped = n.cancel_host(c["s"], c["x"], c["chans"], c["series"], c["amp"], ms_done=c["ms_done"],
                               rec_file_offset=c["off"])
    excluded = cases.compare(name, y, clipped)
    with capsys.disabled():
        print("\n[cancel] %s: %d samples, %d excluded as rounding decisions, %d clipped" % (name, y.size, excluded, clipped))


def test_design_equals_the_contract():
    """smooth 1, 5 and 21 on series of 40 and 12 blocks - both ends of the series are inside every window of 21 - with a zero
    prompt, a prompt pair whose product with its neighbours is exactly 0, ms_done short and 0, and a channel that is off."""
    n = pkg("_native")
    for name, done in (("nearfar", None), ("nearfar", [17, 40]), ("rate2", None), ("rate2", [12, 0, 3]), ("off_done", "own")):
        c = cases.get(name)
        done = c["ms_done"] if done == "own" else done
        series = np.array(c["series"])
        series[0, 3, 5] = series[0, 7, 5] = 0.0              # a zero prompt
        series[0, 3, 2], series[0, 7, 2] = 0.0, 1000.0       # orthogonal to block 3: the sign of 0 counts as +1
        series[0, 3, 3], series[0, 7, 3] = 1000.0, 0.0
        st = spec.states(c["s"], len(c["x"]) + 10 ** 7, c["off"], c["chans"], series, done)
        state = n.replay_state(c["s"], c["chans"], series, ms_done=done)
        for smooth in (1, 5, 21):
            want = spec.design(series, st, done, smooth)
            got = n.cancel_design(series, state, ms_done=done, smooth=smooth)
            assert got.shape == want.shape and np.array_equal(got, want), (name, done, smooth)
            assert np.any(want[0]) and (smooth > 1 or not np.any(want[0, 5]))
    for bad in (0, 2, 4, 43, -1):
        with pytest.raises(n.SgxError) as e:
            n.cancel_design(series, state, ms_done=done, smooth=bad)
        assert e.value.code == n.SGX_E_ARG
        with pytest.raises(ValueError):
            spec.design(series, st, done, bad)


def test_refused_arguments_write_nothing():
    n = pkg("_native")
    L = n.lib()
    c = cases.get("rate2")
    s, x, series, amp = n.settings_struct(c["s"]), c["x"], np.ascontiguousarray(c["series"]), np.ascontiguousarray(c["amp"])
    chans = n._chan_array(c["chans"])
    ms = series.shape[2]

    def refused(code, n_ch=3, ms_done=None, data_type=n.DT_INT8, amp=amp, series=series, count=x.size, off=0, drop=()):
        y = np.full(x.size, 77, dtype=np.int8)
        clipped = C.c_int64(-5)
        done = None if ms_done is None else np.ascontiguousarray(ms_done, dtype=np.int32)
        args = [C.byref(s), n._ptr(x), count, off, C.cast(chans, C.c_void_p), n_ch, ms, None if done is None else n._ptr(done),
                n._ptr(series), data_type, n._ptr(amp), n._ptr(y), C.byref(clipped)]
        for i in drop:
            args[i] = None
        rc = L.sgx_cancel_host(*args)
        assert rc == code, (rc, n.last_error())
        assert np.all(y == 77) and clipped.value == -5

    refused(n.SGX_E_ARG, n_ch=0)
    refused(n.SGX_E_ARG, n_ch=33)
    refused(n.SGX_E_ARG, ms_done=[12, 13, 12])
    refused(n.SGX_E_ARG, ms_done=[-1, 12, 12])
    for dt in (n.DT_UINT8, n.DT_INT16, n.DT_FLOAT32, n.DT_FLOAT64, 77):
        refused(n.SGX_E_ARG, data_type=dt)
    for bad in (float("nan"), float("inf"), -float("inf")):
        a = np.array(amp)
        a[2, 11, 1] = bad
        refused(n.SGX_E_ARG, amp=a)
    for i in (0, 1, 4, 8, 10, 11, 12):
        refused(n.SGX_E_ARG, drop=(i,))
    moved = np.array(series)
    moved[1, 0, 4] += 1.0
    refused(n.SGX_E_ARG, series=moved)                       # (sgx_replay_state's refusals, with its codes)
    refused(n.SGX_E_RANGE, count=int(series[:, 0, -1].max()) - 1)
    refused(n.SGX_E_RANGE, off=int(min(ch[2] for ch in c["chans"])) + 1)
    assert L.sgx_if_cancel(None, None, 0, None, 3, ms, None, None, 0, None, None, None) == n.SGX_E_ARG
    assert L.sgx_cancel_timing(None, None) == n.SGX_E_ARG
    with pytest.raises(ValueError):
        n.cancel_host(c["s"], x, c["chans"], series, amp[:, :5])


def test_near_far_scene_with_oracle_search_and_tracking(capsys):
    """The raw search detects PRN 1 and 3 only; with both cancelled (one amplitude pair per block) the search detects PRN 7
    and 11 within one sample of code phases 4000 and 15000, PRN 14 and 19 (absent) stay below acqThreshold, and the prompt
    power of both cancelled channels, replayed on the cleaned record, falls by at least 25 dB (measured: -33.4 and -31.5 dB;
    the 6 dB between them and the bar cover other noise realisations)."""
    s, rec, raw, chans, series = nf.oracle_run()
    amp, y, v, clipped, covered = nf.oracle_cancelled()
    clean = nf.search(s, y)
    drop = nf.prompt_power_db(s, y, chans, series) - nf.prompt_power_db(s, rec, chans, series)
    with capsys.disabled():
        print("\n[cancel] near-far scene, peakMetric of PRN %s" % (nf.SEARCHED,))
        print("[cancel]   raw     %s" % " ".join("%6.2f" % raw[p][0] for p in nf.SEARCHED))
        print("[cancel]   cleaned %s   code phases %s" % (" ".join("%6.2f" % clean[p][0] for p in nf.SEARCHED),
                                                         [int(clean[p][1]) for p in nf.WEAK]))
        print("[cancel]   prompt power of the cancelled channels: %+.1f and %+.1f dB; %d of %d outputs clipped, %.2f %% of the "
              "inputs on a rail" % (drop[0], drop[1], clipped, y.size, 100.0 * np.mean(np.abs(rec.astype(np.int16)) >= 127)))
    assert nf.detected(raw, s) == [1, 3]
    found = nf.detected(clean, s)
    assert 7 in found and 11 in found and 14 not in found and 19 not in found
    assert abs(clean[7][1] - 4000) <= 1 and abs(clean[11][1] - 15000) <= 1
    assert clean[14][0] < s.acqThreshold and clean[19][0] < s.acqThreshold
    assert np.all(drop <= -25.0), drop


def test_near_far_scene_behind_the_conditioning_stage_with_the_oracle(capsys):
    """The claims of the resident path (tests/test_cancel_gpu.py) on the CPU: the scene's file carries a DC offset of 5 LSB,
    the prepared record is the conditioning stage's numpy contract on it (the default settings: the offset removed, the rms
    brought to 12 LSB); there the oracle's search detects PRN 1 and 3, and with both tracked and cancelled by the contract
    its search of the cleaned record detects, of the PRNs that are not tracked, PRN 7 and 11 and no other."""
    s = nf.settings()
    prepared = nf.prepared_record()
    assert abs(float(nf.offset_file().mean()) - nf.DC_OFFSET) < 0.5 and abs(float(prepared.mean())) < 0.05
    assert abs(float(prepared.std()) - nf.COND["condTargetRms"]) < 0.5
    assert prepared.size == nf.MS_TRACKED * (s.samplesPerCode + 2) + 2 * s.samplesPerCode      # what postProcessing() reads
    raw, chans, series, clean = nf.oracle_run_prepared()
    with capsys.disabled():
        print("\n[cancel] behind the conditioning stage, peakMetric of PRN %s: raw %s, cleaned %s, code phases %s" % (
            nf.SEARCHED, " ".join("%.2f" % raw[p][0] for p in nf.SEARCHED), " ".join("%.2f" % clean[p][0] for p in nf.SEARCHED),
            [int(clean[p][1]) for p in nf.WEAK]))
    assert nf.detected(raw, s) == [1, 3] and [c[0] for c in chans] == [1, 3]
    assert [p for p in nf.detected(clean, s) if p not in nf.STRONG] == [7, 11]
    assert abs(clean[7][1] - 4000) <= 1 and abs(clean[11][1] - 15000) <= 1


def test_settings_and_command_line_surface():
    """Off by default; the options are refused together as the usage says, before anything is opened."""
    m = pkg()
    s = m.Settings()
    assert s.strongSignalCancellation is False and s.cancelCNoThreshold == 60.0 and s.cancelSmoothMs == 1
    main = pkg("main").main
    for argv in (["x.bin", "--cancel-smooth", "3"], ["x.bin", "--cancel-strong", "--cancel-smooth", "4"],
                 ["x.bin", "--cancel-strong", "--cancel-smooth", "43"], ["x.bin", "--cancel-strong=nan"]):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2, argv
    for name in ("cancel", "join"):
        assert callable(getattr(m.TrackingResult, name))
    assert callable(m._native.Context.if_cancel) and callable(m._native.Context.cancel_timing)


def test_host_code_under_sanitizers(tmp_path):
    """tools/cancel_check.cpp, a program of its own, built with AddressSanitizer and UBSan from the host sources only and run
    on the CPU: the design and the host twin on a record that ends with the last block's last sample."""
    cxx = shutil.which("g++")
    assert cxx, "no g++ for the host build"
    exe = str(tmp_path / "cancel_check")
    csrc = os.path.join(ROOT, "softgnss-python_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tools", "cancel_check.cpp"),
                    os.path.join(csrc, "sgx_cancel.cpp"), os.path.join(csrc, "sgx_core.cpp"), "-o", exe, "-lm"], check=True)
    # (the runtimes are linked into the program: it needs nothing preloaded)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "no report" in text, text
