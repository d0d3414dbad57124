"""CPU-only checks of the dense coherent-acquisition cases (tests/dense_scene.py) that tests/test_coherent_acq_gpu.py
asserts exactly on the GPU: each scene is placed as designed, and each search is well-conditioned in the numpy contract
alone (tests/coherent_acq_spec.py) - every placed satellite detected on its bin with room to spare, and no asserted
arg-max within 1e-6 (relative) of its runner-up.  1e-6 is a condition, three orders above the 1e-9 allowed on peakMetric.

Run time of each case's contract (8 CPU workers; the GPU job's time limits are sized from these):
  2x2_offset 4 s, 2x2_noncoh_f64_29 4 s, 10x2_ref 19 s, 10x2_noncoh 18 s, 2x20_windows 9 s, 20x2_a 38 s, 20x2_b 35 s,
  5x64_noncoh 22 s, rate2_4x2_ref 2 s, rate2_4x2_noncoh 2 s, fs5456_2x3 1 s, if3000_2x2 2 s (156 s in all).
"""
import time

import numpy as np
import pytest

import coherent_acq_spec as spec
import dense_scene
import weak_scene

GAP = 1e-6
CASE_IDS = [c.name for c in dense_scene.CASES]


@pytest.mark.parametrize("name", CASE_IDS)
def test_scene_is_placed_as_designed(name):
    c = dense_scene.BY_NAME[name]
    g, rows = c.g, c.sats()
    N = c.s.samplesPerCode
    spc = int(round(c.s.samplingFreq / c.s.codeFreqBasis))
    assert sorted(r["prn"] for r in rows) == sorted(c.prns) and len(set(c.prns)) == len(c.prns)
    bins = [r["bin"] for r in rows]
    assert g["n_bins"] - 1 in bins
    assert (0 in bins) or c.min_freq is not None
    for r in rows:
        assert abs(r["off"]) <= 0.3
        assert r["doppler"] == g["freqs"][r["bin"]] + r["off"] * g["step"] - c.s.IF
        if r["bin"] in (0, g["n_bins"] - 1):
            assert r["off"] == 0.0 and abs(r["doppler"]) == c.s.acqSearchBand * 500.0 or c.min_freq is not None
        assert spc + 2 <= r["phase"] < N - spc - 2
        if c.min_freq is not None:
            assert g["freqs"][r["bin"]] + r["off"] * g["step"] > c.min_freq
    on_bin = sum(r["off"] == 0.0 for r in rows)
    assert len(rows) // 2 - 2 <= on_bin <= len(rows) // 2 + 4, on_bin
    assert min(r["phase"] for r in rows) <= spc + 2 + 3 and max(r["phase"] for r in rows) >= N - spc - 2 - 3
    if g["path"] == "shift":
        hit = set(g["phi_index"][k] for k in bins)
        if g["n_phi"] + 3 <= len(rows):
            assert hit == set(range(g["n_phi"]))
        if g["n_phi"] >= 2:
            assert any(g["phi_index"][a] == g["phi_index"][b] and g["shift"][a] != g["shift"][b] for a in bins for b in bins)
    for k in dense_scene.cut_bins(g):
        assert k in bins, k
    for r in rows:
        if r["protected"]:
            assert r["prn"] not in c.drop
    assert len(c.drop) <= 2 and set(c.no_fine) <= set(r["prn"] for r in rows if "on" in r)
    assert (g["path"], g["prn_chunk"], g["bin_runs"]) == (c.path, c.prn_chunk, c.bin_runs)


def test_the_two_twenty_ms_scenes_hit_every_phi_row():
    a, b = dense_scene.BY_NAME["20x2_a"], dense_scene.BY_NAME["20x2_b"]
    hit = set(a.g["phi_index"][r["bin"]] for r in a.sats() + b.sats())
    assert a.g["n_phi"] == 40 and hit == set(range(40))


def test_window_gates_sit_on_both_sides_of_the_cut():
    c = dense_scene.BY_NAME["2x20_windows"]
    assert c.g["per_run"] == 16 and c.g["bin_runs"] == 2
    on = sorted(r["on"] for r in c.sats() if "on" in r)
    assert on == [(0, 2), (30, 32), (30, 32), (32, 34), (32, 34), (38, 40)]     # windows 0, 15, 15, 16, 16, 19


def test_details_do_not_change_the_search():
    sats = ((1, 52.0, 210.0, 5000), (6, 50.0, -380.0, 20000))
    s = dense_scene.settings(band=1.0)
    x = weak_scene.generate(12, sats=sats, seed=7)
    plain = spec.acquire(s, x, 2, 2, False, None, prn_indices=[1, 6, 9])
    full = spec.acquire(s, x, 2, 2, False, None, prn_indices=[1, 6, 9], details=True)
    for k in plain:
        assert np.array_equal(plain[k], full[k]), k
    d = full["details"][1]
    assert d["bins"][0][1] == full["freqBin"][1] and d["samples"][0][1] == full["codePhase"][1]
    assert d["fine"][0][1] - 4 == full["fineIdx"][1] and len(d["window"]) == 5
    par = dense_scene.parallel_spec(s, x, 2, 2, False, None, [1, 6, 9], workers=2)
    for k in plain:
        assert np.array_equal(plain[k], par[k]), k


@pytest.mark.parametrize("direct", [False, True])
def test_index_error_records(direct):
    """The contract raises the reference's IndexError for a peak at code phase spc exactly, and only there: the control
    record (peak at sample 11) is searched to the end."""
    o, kw, p = dense_scene.index_error_case(direct)
    assert spec.grid(o, 2, 2, False, None)["path"] == ("direct" if direct else "shift")
    with pytest.raises(IndexError):
        spec.acquire(o, dense_scene.index_error_record(o), 2, 2, False, None, prn_indices=[p])
    w = spec.acquire(o, dense_scene.index_error_record(o, control=True), 2, 2, False, None, prn_indices=[p], details=True)
    assert w["codePhase"][p] == 11 and w["peakMetric"][p] > 10
    assert min(spec.rel_gap(w["details"][p][k]) for k in ("bins", "samples", "fine")) >= GAP


def conditioning(c, ref):
    """{PRN index: (smallest relative gap, which)} over the arg-maxes the GPU test asserts for it."""
    out = {}
    for p in c.prns:
        d = ref["details"][p]
        gaps = [(spec.rel_gap(d["bins"]), "bin"), (spec.rel_gap(d["samples"]), "sample")]
        if d["fine"] is not None:
            gaps.append((spec.rel_gap(d["fine"]), "fine"))
        out[p] = gaps
    return out


@pytest.mark.slow
@pytest.mark.parametrize("name", CASE_IDS)
def test_case_is_well_conditioned(name):
    c = dense_scene.BY_NAME[name]
    x = c.record()
    assert x.dtype == np.int8 and int(np.abs(x.astype(np.int16)).max()) < 127
    t0 = time.time()
    ref = c.reference()
    print("\n%s: spec %.0f s" % (name, time.time() - t0))
    rows = {r["prn"]: r for r in c.sats()}
    cond = conditioning(c, ref)
    worst = {}
    for p in c.prns:
        r = rows[p]
        lo, hi = c.phase_range(r)
        print(p, r["bin"], ref["freqBin"][p], r["phase"], ref["codePhase"][p], "%.2f" % ref["peakMetric"][p],
              ["%s %.1e" % (w, gp) for gp, w in cond[p]])
        assert ref["peakMetric"][p] >= 1.2 * c.s.acqThreshold, (p, ref["peakMetric"][p])
        assert ref["carrFreq"][p] > 0
        assert ref["freqBin"][p] == r["bin"], (p, ref["freqBin"][p], r["bin"])
        assert lo - 2 <= ref["codePhase"][p] <= hi + 2, (p, ref["codePhase"][p], lo, hi)
        for gp, which in cond[p]:
            if gp < GAP:
                worst[(p, which)] = gp
    fine_only = {p: gp for (p, which), gp in worst.items() if which == "fine" and p in c.no_fine}
    other = {p: gp for (p, which), gp in worst.items() if not (which == "fine" and p in c.no_fine)}
    assert set(other) <= set(c.drop), other
    assert set(fine_only) <= set(c.no_fine), fine_only
