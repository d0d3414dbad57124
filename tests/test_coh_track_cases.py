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
from conftest import ROOT, pkg
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
