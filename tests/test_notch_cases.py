"""The jammed scene of the interference-excision tests is well-conditioned by the reference alone (numpy + oracle, no
library): a continuous-wave line of 100 LSB at IF + 180 kHz (phase 0.3 rad, clipped to +-127) hides satellites from the
reference's acquisition, and the CONTRACT's own detect + design + apply (tests/notch_spec.py: 80 kHz, 1025 taps, Q14) brings
all eight back with a margin of 1.2 either side of the threshold.  Measured with these values: raw metrics 2.14 2.62 3.99
1.01 3.25 3.18 2.61 1.01 (5 of 8 detected), mitigated 7.3 .. 16.0, absent PRNs 5 and 9 at 1.09 and 1.34."""
import numpy as np
import pytest

import notch_cases as cases
import notch_spec as spec
from oracle import softgnss_oracle as orc


@pytest.fixture(scope="module")
def searches():
    s = orc.OracleSettings()
    n = 11 * s.samplesPerCode
    raw = cases.jammed(10)[:n]
    lines, f = cases.contract_lines(raw, s)
    taps = spec.design(lines, s.samplingFreq, cases.TAPS)
    clean = spec.apply(raw, taps, spec.DESIGN_SHIFT)
    return s, raw, lines, f, orc.acquire(s, raw), orc.acquire(s, clean)


def test_exactly_one_line_at_the_jammer(searches):
    s, raw, lines, f, _, _ = searches
    assert 0.03 < np.mean(np.abs(raw.astype(int)) == 127) < 0.05       # the jammer saturates about 4 % of the samples
    assert len(lines) == 1
    assert abs(lines[0][0] - (s.IF + cases.CW_OFFSET_HZ)) <= (f[1] - f[0]) * 1e6
    assert lines[0][1] == cases.WIDTH_HZ


def test_the_jammer_hides_satellites_from_the_reference(searches):
    s, _, _, _, before, _ = searches
    idx = [p - 1 for p in cases.PRESENT]
    assert np.count_nonzero(before["carrFreq"][idx]) <= 6


def test_the_contract_notch_brings_all_eight_back(searches):
    s, _, _, _, _, after = searches
    idx = [p - 1 for p in cases.PRESENT]
    assert np.all(after["carrFreq"][idx] != 0)
    assert np.all(after["peakMetric"][idx] >= cases.MARGIN * s.acqThreshold), after["peakMetric"][idx]
    absent = [p - 1 for p in cases.ABSENT]
    assert np.all(after["peakMetric"][absent] <= s.acqThreshold / cases.MARGIN), after["peakMetric"][absent]
    assert sorted(np.flatnonzero(after["carrFreq"]) + 1) == list(cases.PRESENT)


def test_the_clean_scene_has_no_line():
    lines, _ = cases.contract_lines(cases.clean(10))
    assert lines == []
