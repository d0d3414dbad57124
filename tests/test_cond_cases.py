"""The end-to-end scene of tests/cond_cases.py shown on the CPU with the contracts and the oracle alone: through the
fixed-gain requantiser (tests/requant_spec.py) and the converter the oracle's acquisition loses the satellites; through the
conditioning stage (tests/cond_spec.py) and the same converter it finds all eight with the margin of tests/iq_cases.py."""
import math

import numpy as np

import cond_cases as cases
import iq_cases
import requant_spec


def test_the_fixed_gain_chain_fails_the_scene():
    scene = cases.SCENE
    x = cases.capture()
    y8, mult, shift = cases.fixed_gain_record()
    st = requant_spec.stats(x, x.dtype)
    clipped = requant_spec.clipped_share(y8)
    ref = cases.acquisition("fixed")
    o = scene.oracle_settings()
    found = [p for p in scene.prns if ref["carrFreq"][p - 1] != 0.0
             and abs(ref["carrFreq"][p - 1] - scene.true_carrier(scene.prns.index(p))) <= iq_cases.CARR_TOL_HZ]
    print("fixed gain: rms %.1f, mult %d, shift %d (%.2f dB), clipped share %.3g, found %r"
          % (math.sqrt(st["sum_sq"] / st["n_finite"]), mult, shift, 20.0 * math.log10(mult / 2.0 ** shift), clipped, found))
    print("peak metric / threshold:", [round(float(ref["peakMetric"][p - 1]) / o.acqThreshold, 2) for p in scene.prns])
    assert len(found) <= len(scene.prns) - 2 or clipped > cases.MAX_CLIPPED


def test_the_conditioned_chain_finds_all_eight():
    scene = cases.SCENE
    x = cases.capture()
    st, plan, y8, blanked, clipped = cases.conditioned()
    frames = x.size // 2
    print("conditioned: %d blocks of %d frames, %.3f %% of the frames blanked, %.3g of the samples clipped"
          % (plan.size, cases.BLOCK, 100.0 * blanked / frames, clipped / x.size))
    assert clipped / x.size <= cases.MAX_CLIPPED and 0.02 <= blanked / frames <= 0.10
    # the level on either side of the step, and the DC gone
    n = scene.samples_per_code
    for lo, hi in ((0, 100 * n), (200 * n, 300 * n)):
        seg = y8[lo:hi].astype(np.float64)
        keep = seg != 0
        assert abs(float(np.sqrt(np.mean(seg[keep] ** 2))) - cases.TARGET_RMS) < 1.0
        assert abs(float(seg[0::2].mean())) < 0.2 and abs(float(seg[1::2].mean())) < 0.2
    ref = cases.acquisition("conditioned")
    o = scene.oracle_settings()
    assert sorted(np.flatnonzero(ref["carrFreq"]) + 1) == sorted(scene.prns)
    for i, prn in enumerate(scene.prns):
        f, c, pm = ref["carrFreq"][prn - 1], ref["codePhase"][prn - 1], ref["peakMetric"][prn - 1]
        print("PRN %2d: carrFreq %+.1f Hz, code phase %+.2f samples off the truth, peak metric / threshold %.2f"
              % (prn, f - scene.true_carrier(i), c - scene.code_start[i], pm / o.acqThreshold))
        assert abs(f - scene.true_carrier(i)) <= iq_cases.CARR_TOL_HZ
        assert abs(c - scene.code_start[i]) <= iq_cases.PHASE_TOL
        assert pm >= iq_cases.MARGIN * o.acqThreshold
