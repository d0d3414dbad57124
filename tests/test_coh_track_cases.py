"""CPU checks of the coherent-tracking contract (tests/coh_track_spec.py) and of the scenes the GPU tests run on
(tests/coh_track_cases.py): the spec is anchored to the oracle, the fade scene shows in numpy alone what the feature is for,
and every scene whose bit edge the kernel has to find has a clear margin - so the GPU tests cannot hide behind a scene.
No kernel runs here."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import coh_track_cases as cases
import coh_track_spec as spec
from conftest import ROOT, load_golden, pkg
from oracle import softgnss_oracle as orc

F_SEEDS = cases.F_SEEDS           # 1 .. 6: the generator as committed meets every condition on all six


def test_spec_equals_the_oracle_while_nothing_is_coherent():
    """T = 1, and T = 20 with the pull-in as long as the run: oracle.track, bit for bit."""
    ms = 200
    s, rec, chans, _ = cases.scene_trio(ms)
    chans = chans[:2]
    s.numberOfChannels = 2
    table = dict(PRN=np.array([c[0] for c in chans]), acquiredFreq=np.array([c[1] for c in chans]),
                 codePhase=np.array([c[2] for c in chans]), status=np.array(["T", "T"]))
    want = orc.stack_series(orc.track(s, table, rec, ms))
    for T, P, edges in ((1, 40, [3, 5]), (20, ms, [3, 5]), (20, ms, [0, -1])):
        got = spec.track(s, chans, rec, ms, T, P, 100, edges)
        assert np.array_equal(got["ms_done"], [ms, ms])
        assert np.array_equal(got["series"], want), (T, P, edges)
    assert np.array_equal(spec.track(s, chans, rec, ms, 1, 40, 100, [3, 5])["k0"], [-1, -1])
    assert np.array_equal(spec.track(s, chans, rec, ms, 20, ms, 100, [0, 5])["k0"], [200, 205])


@pytest.fixture(scope="module", params=F_SEEDS)
def fade(request):
    s, rec, bits, ch = cases.scene_f(request.param)
    coh = spec.track(s, [ch], rec, cases.F_MS, 20, 600, 100, [-1], coh_pll_bw=3.0, coh_dll_bw=1.0)
    ref = spec.track(s, [ch], rec, cases.F_MS, 1, 600, 100, [cases.F["edge"]])
    return bits, coh, ref


def test_fade_scene_coherent_loops_keep_the_signal(fade):
    bits, coh, _ = fade
    assert coh["ms_done"][0] == cases.F_MS
    assert coh["edge"][0] == cases.F["edge"] and coh["k0"][0] == 607
    assert cases.edge_margin(coh["energy"][0]) >= 1.05
    ser = coh["series"][0]
    assert cases.wrong_bits(ser[3], bits, cases.F["edge"], cases.F_MS - 1500) == 0.0
    truth = cases.IF_LOW + cases.F["doppler"]
    assert np.max(np.abs(ser[2, -1000:] - truth)) < 10.0


def test_fade_scene_reference_loops_lose_it(fade):
    bits, _, ref = fade
    assert ref["ms_done"][0] == cases.F_MS
    assert cases.wrong_bits(ref["series"][0][3], bits, cases.F["edge"], cases.F_MS - 1500) >= 0.20


@pytest.mark.parametrize("P,skip", cases.SYNC_SCENES)
def test_bit_sync_scenes_have_a_margin(P, skip):
    """Every found-edge run of the GPU file on the three-satellite scene (seed cases.TRIO_SEED = 12; the fade scene's are
    the tests above)."""
    s, rec, chans, edges = cases.scene_sync(skip)
    got = spec.track(s, chans, rec, cases.SYNC_MS, 20, P, 100, [-1, -1, -1, -1])
    assert np.array_equal(got["edge"][:3], edges[:3])
    assert np.array_equal(got["k0"][:3], [spec.first_group_start(P, e) for e in edges[:3]])
    for c in range(3):
        assert cases.edge_margin(got["energy"][c]) >= 1.05, (P, c)
    assert got["ms_done"][3] == 0 and got["k0"][3] == -1


# ---- the limits (tests/test_coh_track_limits_gpu.py): what each case's table claims, and that the nearest wrong result of
# each lies outside the GPU test's bar - conditions on the inputs, by the contract alone ------------------------------------

BAR = 1e-9                        # tests/test_coh_track_gpu.py: TOL
_MEMO = {}


def _once(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def _trio():
    return _once("trio", lambda: cases.scene_trio(cases.SYNC_MS))


def _apart(a, b, rows):
    """The largest |delta| of the six sums over RMS |P|, the scale of the GPU test's bar, over the channels `rows`."""
    worst = 0.0
    for c in rows:
        rms = max(1.0, float(np.sqrt(np.mean(a["series"][c, 3] ** 2 + a["series"][c, 7] ** 2))))
        worst = max(worst, float(np.max(np.abs(a["series"][c, 3:9] - b["series"][c, 3:9]))) / rms)
    return worst


def _locked(w, rows, lo=3.0e3):
    """Mean |I_P| of the last 30 blocks well above the noise's (sigma sqrt(4092 / 2) = 900; the signal's is 7.2e3)."""
    return all(float(np.mean(np.abs(w["series"][c, 3, -30:]))) > lo for c in rows)


@pytest.mark.parametrize("fs,IF,units,by_sample", cases.RATE_SCENES)
def test_rate_scenes_are_what_their_table_says(fs, IF, units, by_sample):
    """Case 1: the units and the map by the formulas of csrc/sgx_trk.hip, the run complete, locked and coherent from the
    trio's k0 on - and its groups show: the same run with every block updated lies far outside the bar."""
    s, rec, chans, edges = cases.scene_trio(cases.RATE_RUN["ms"], fs, IF)
    assert cases.trk_units(s.samplesPerCode) == units <= 16 and cases.trk_by_sample(fs) == by_sample
    assert cases.trk_units(s.samplesPerCode + 4096) > units or units == 16
    w = spec.track(s, chans, rec, edges=edges, **cases.RATE_RUN)
    assert list(w["ms_done"]) == [110, 110, 110, 0] and list(w["k0"]) == [40, 47, 59, -1]
    level = [float(np.mean(np.abs(w["series"][c, 3, -30:]))) for c in range(3)]
    assert 6.5e3 <= min(level) and max(level) < 2.45e4, level        # (6.51e3 .. 2.445e4 over the four rates)
    plain = spec.track(s, chans, rec, edges=edges, **dict(cases.RATE_RUN, T=1))
    assert _apart(w, plain, range(3)) > 1e-3
    if fs == 16.368e6:             # (the GPU test runs this rate at T = 4 as well: groups that end inside a bit)
        w4 = spec.track(s, chans, rec, edges=edges, **dict(cases.RATE_RUN, T=4))
        assert list(w4["ms_done"]) == [110, 110, 110, 0] and list(w4["k0"]) == [40, 47, 59, -1] and _apart(w4, w, range(3)) > 1e-3


def test_offset_scenes():
    """Case 2: a moved channel keeps its code phase and its true edge; a record that starts `off` bytes into the file is the
    same run with absoluteSample `off` larger - exactly, also 2^33 + 4096 - and a result that dropped the offset, kept 32 bits
    of it or read one byte beside its place is outside the bar."""
    s, rec, chans, edges = _trio()
    base = spec.track(s, chans, rec, edges=edges, **cases.OFFSET_RUN)
    for name in ("window", "odd"):
        off = cases.OFFSETS[name]
        moved, e2 = cases.moved_behind(chans, edges, off)
        assert all(c[2] >= off for c in moved[:3]) and (moved[0][2] - chans[0][2]) % 4092 == 0 and moved[3] == chans[3]
        assert e2[0] == (edges[0] - (moved[0][2] - chans[0][2]) // 4092) % 20
        want = spec.track(s, moved, rec, edges=e2, **cases.OFFSET_RUN)
        assert list(want["ms_done"]) == [110, 110, 110, 0] and _locked(want, range(3))
        assert list(want["k0"][:3]) == [spec.first_group_start(40, e) for e in e2[:3]]
        # the window alone, positions counted from its first byte: the same but for absoluteSample, which is `off` smaller
        part = spec.track(s, [(p, f, cp - off if p else cp) for p, f, cp in moved], rec[off:], edges=e2, **cases.OFFSET_RUN)
        assert np.array_equal(part["series"][:, 1:], want["series"][:, 1:]) and np.array_equal(part["energy"], want["energy"])
        assert np.array_equal(part["series"][:3, 0] + off, want["series"][:3, 0])
        assert np.all(part["series"][:3, 0] != want["series"][:3, 0])                       # the offset dropped
        beside = spec.track(s, [(p, f, cp + 1 if p else cp) for p, f, cp in moved], rec, edges=e2, **cases.OFFSET_RUN)
        assert _apart(beside, want, range(3)) > 1e-3                                          # a read one byte off
    big = cases.OFFSETS["large"]
    pos = base["series"][:3, 0]
    assert big % 16 == 0 and np.all((pos + big) - big == pos) and np.all(pos + big != pos + big % 2 ** 32)
    # 2(e): the edges are found on the moved scene, each with a margin
    moved, e2 = cases.moved_behind(chans, edges, cases.OFFSETS["classes"])
    sync = _once("classes", lambda: spec.track(s, moved, rec, edges=[-1] * 4, **cases.OFFSET_SYNC))
    assert list(sync["edge"][:3]) == e2[:3] and list(sync["ms_done"]) == [400, 400, 400, 0]
    assert list(sync["k0"][:3]) == [spec.first_group_start(300, e) for e in e2[:3]]
    assert all(cases.edge_margin(sync["energy"][c]) >= 1.05 for c in range(3))


def test_many_channels_cannot_be_mixed_up():
    """Case 4: 294 active rows that all complete, with 294 values of I_P[59] that lie farther apart than the bar."""
    s, rec, chans, edges = _trio()
    rows, ed = cases.many_channels(chans, edges)
    assert len(rows) == 300 and [i for i, r in enumerate(rows) if r[0] == 0] == list(cases.MANY_OFF)
    w = _once("many", lambda: spec.track(s, rows, rec, edges=ed, **cases.MANY_RUN))
    act = np.array([i for i in range(300) if i not in cases.MANY_OFF])
    assert np.all(w["ms_done"][act] == 60) and np.all(w["ms_done"][list(cases.MANY_OFF)] == 0)
    assert np.array_equal(w["k0"][act], [spec.first_group_start(40, ed[i]) for i in act])
    last = np.sort(w["series"][act, 3, 59])
    rms = float(np.sqrt(np.mean(w["series"][act, 3] ** 2 + w["series"][act, 7] ** 2)))
    assert len(set(last)) == 294 and np.min(np.diff(last)) > 100 * BAR * rms
    # (the first 65 rows, the GPU test's second call, are the same rows: a channel's result does not depend on the table)
    assert len(set(ed[:65])) == 20 and sum(r[0] != 0 for r in rows[:65]) == 62


@pytest.mark.parametrize("fs,IF", cases.FULL_SCALE_RATES)
def test_full_scale_scenes(fs, IF):
    """Case 5: both records complete with k0 = 43 at a level no other scene reaches; the clipped one holds -128 and 127 and
    nothing else, and -128 read as 128 moves I_P by about its own size."""
    m = pkg()
    for kind in ("clipped", "clean"):
        s, rec, ch = cases.full_scale_case(m, fs, IF, kind)
        w = spec.track(s, ch, rec, edges=[cases.FULL_SCALE_EDGE], **cases.FULL_SCALE_RUN)
        assert list(w["ms_done"]) == [100] and list(w["k0"]) == [43]
        level = float(np.mean(np.abs(w["series"][0, 3, -30:])))
        assert level > (2.0e5 if fs < 1.0e7 else 2.0e6), level
        if kind == "clean":
            assert rec.min() == -127 and rec.max() == 127
            continue
        assert sorted(set(rec.tolist())) == [-128, 127]
        wide = rec.astype("<i2")
        wide[wide == -128] = 128
        s16 = cases.settings(fs, IF, dataType="int16")
        wrong = spec.track(s16, [(ch[0][0], ch[0][1], 2 * ch[0][2])], wide, edges=[cases.FULL_SCALE_EDGE], **cases.FULL_SCALE_RUN)
        assert list(wrong["ms_done"]) == [100] and _apart(wrong, w, [0]) > 0.5


def test_t1_scene_has_a_margin():
    """Case 6: T = 1 with the edges found - the true ones, each with a margin - and no coherent phase."""
    s, rec, chans, edges = _trio()
    w = spec.track(s, chans, rec, edges=[-1] * 4, **cases.T1_RUN)
    assert list(w["edge"]) == edges[:3] + [-1] and list(w["k0"]) == [-1] * 4 and list(w["ms_done"]) == [300, 300, 300, 0]
    assert all(cases.edge_margin(w["energy"][c]) >= 1.05 for c in range(3))


def test_channels_that_end_while_the_edge_is_sought():
    """Case 7: no edge, no k0, and energies that are not zero - so a kernel that left them out, or zeroed them, shows."""
    s, rec, chans, edges = _trio()
    for how, done in (("silence", [101, 101, 101, 0]), ("short", [150, 149, 149, 0])):
        w = spec.track(s, chans, cases.ends_early(rec, chans, how), edges=[-1] * 4, **cases.ENDS_RUN)
        assert list(w["ms_done"]) == done and list(w["edge"]) == [-1] * 4 and list(w["k0"]) == [-1] * 4
        top = w["energy"][:3].max(axis=1)
        assert np.all(top > 5e10) and np.all(top < 5e11) and np.all(w["energy"][3] == 0.0)
        assert np.all(np.sum(w["energy"][:3] > 0, axis=1) == 20)
        if how == "silence":
            for c in range(3):
                assert np.isnan(w["series"][c, 1, 100]) and np.all(w["series"][c, 3:9, 100] == 0.0)


def test_range_scene_fits_at_2_khz_and_not_at_6():
    """Case 8: the longest block of the contract against the ten units of the launch less the worst alignment."""
    m = pkg()
    rec = m.synth.generate(m.synth.Scene.default(), m.synth.record_length(38192, 80))
    first = np.array([[c[2]] for c in cases.RANGE_CHANNELS])
    for bw, longest, at in ((2000.0, 39239, None), (6000.0, 43120, 28)):
        s = cases.settings(38.192e6, 9.548e6, dllNoiseBandwidth=bw)
        w = spec.track(s, cases.RANGE_CHANNELS, rec, edges=[0, 0], **cases.RANGE_RUN)
        assert list(w["ms_done"]) == [60, 60]
        blocks = np.diff(np.concatenate([first, w["series"][:, 0]], axis=1), axis=1)
        assert blocks.max() == longest
        if at is None:
            assert longest <= cases.RANGE_ROOM
        else:
            assert np.all(blocks[0] <= cases.RANGE_ROOM) and int(np.argmax(blocks[1] > 10 * 4096)) == at


@pytest.mark.parametrize("loops", cases.LOOPS)
def test_other_loops_show(loops):
    """Case 9: both settings complete, locked, and lie far outside the bar of the same run with the default coherent
    bandwidths (a kernel that took the coherent coefficients from the defaults) and of the default 1 ms loops."""
    s0, rec, chans, edges = _trio()
    s = cases.settings(**loops)
    w = spec.track(s, chans, rec, edges=edges, coh_pll_bw=8.0, coh_dll_bw=0.5, **cases.LOOPS_RUN)
    assert list(w["ms_done"]) == [150, 150, 150, 0] and _locked(w, range(3))
    assert _apart(w, spec.track(s, chans, rec, edges=edges, **cases.LOOPS_RUN), range(3)) > 1e-3
    assert _apart(w, spec.track(s0, chans, rec, edges=edges, coh_pll_bw=8.0, coh_dll_bw=0.5, **cases.LOOPS_RUN), range(3)) > 1e-3


def test_quarter_chip_at_the_default_front_end(default_record):
    g = load_golden("trk_default.npz")
    chans = [(int(g["ch_PRN"][i]), float(g["ch_acquiredFreq"][i]), float(g["ch_codePhase"][i])) for i in range(2)]
    s = cases.settings(38.192e6, 9.548e6, **cases.LOOPS[0])
    w = spec.track(s, chans, default_record, edges=[3, 11], coh_pll_bw=8.0, coh_dll_bw=0.5, **cases.LOOPS_DEFAULT_RUN)
    assert list(w["ms_done"]) == [120, 120] and list(w["k0"]) == [43, 51]
    assert _apart(w, spec.track(s, chans, default_record, edges=[3, 11], **cases.LOOPS_DEFAULT_RUN), range(2)) > 1e-3
    half = cases.settings(38.192e6, 9.548e6)
    assert _apart(w, spec.track(half, chans, default_record, edges=[3, 11], coh_pll_bw=8.0, coh_dll_bw=0.5,
                                **cases.LOOPS_DEFAULT_RUN), range(2)) > 1e-3


def test_cancellation_scene():
    """Case 10: the trio in a record at file offset 4096, its channels (all three start in front of it) moved one code
    period on; all three locked."""
    s, rec, chans, edges = _trio()
    moved, e2 = cases.moved_behind(chans, edges, cases.CANCEL_OFF)
    assert [c[2] - d[2] for c, d in zip(moved, chans)] == [4092, 4092, 4092, 0] and e2 == [19, 6, 18, 0]
    w = spec.track(s, moved, rec, edges=e2, **cases.CANCEL_RUN)
    assert list(w["ms_done"]) == [110, 110, 110, 0] and _locked(w, range(3))


def test_settings_defaults():
    s = pkg().Settings()
    assert (s.trackCoherentMs, s.trackPullInMs, s.trackHandOverMs) == (1, 1000, 100)
    assert (s.cohPllNoiseBandwidth, s.cohDllNoiseBandwidth) == (3.0, 1.0)


def test_main_flags(monkeypatch):
    seen = {}

    def fake(self, fileNameStr=None):
        seen.update(T=self.trackCoherentMs, P=self.trackPullInMs, H=self.trackHandOverMs, pll=self.cohPllNoiseBandwidth,
                    dll=self.cohDllNoiseBandwidth)
        return None, None, None
    monkeypatch.setattr(pkg("initialize").Settings, "postProcessing", fake)
    main = pkg("main").main
    main(["x.bin", "--no-probe", "--track-coherent-ms", "20", "--track-pull-in-ms", "600", "--coh-pll-bw", "2.5"])
    assert seen == dict(T=20, P=600, H=100, pll=2.5, dll=1.0)
    main(["x.bin", "--no-probe"])
    assert seen == dict(T=1, P=1000, H=100, pll=3.0, dll=1.0)
    for bad in (["--track-coherent-ms", "3"], ["--track-pull-in-ms", "600"], ["--track-coherent-ms", "20", "--track-pull-in-ms", "100"],
                ["--track-coherent-ms", "20", "--coh-pll-bw", "0"]):
        with pytest.raises(SystemExit):
            main(["x.bin", "--no-probe"] + bad)


def test_coh_params_layout_matches_the_header():
    importlib.import_module("__graft_entry__").build()
    n = pkg()._native
    text = open(os.path.join(ROOT, "include", "sgx.h")).read()
    body = re.search(r"typedef struct sgx_coh_params \{(.*?)\} sgx_coh_params;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared, off = [], 0
    for kind, names in re.findall(r"\b(double|int32_t)\s+([^;]+);", body):
        for name in names.split(","):
            name = name.strip()
            count = int(re.search(r"\[(\d+)\]", name).group(1)) if "[" in name else 1
            size = 8 if kind == "double" else 4
            off = (off + size - 1) // size * size
            declared.append((name.split("[")[0], off))
            off += size * count
    assert off == 64 and ctypes.sizeof(n.CohParams) == 64
    assert declared == [(name, getattr(n.CohParams, name).offset) for name, _ in n.CohParams._fields_]
    p = n.coh_params(pkg().Settings(), coherent_ms=20)
    assert (p.coherent_ms, p.pull_in_ms, p.handover_ms) == (20, 1000, 100)
    assert (p.tau1_pll, p.tau2_pll) == orc.calc_loop_coef(3.0, 0.7, 0.25)
    assert (p.tau1_dll, p.tau2_dll) == orc.calc_loop_coef(1.0, 0.7, 1.0)
    assert "sgx_track_coherent" in n.SYMBOLS
