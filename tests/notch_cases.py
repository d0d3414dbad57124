"""The jammed scene of the interference-excision tests: the default synthetic scene plus one continuous-wave line inside
the C/A main lobe, and the contract's own mitigation of it (tests/notch_spec.py on the oracle's probe statistics).  Shared
by tests/test_notch_cases.py (CPU, the reference alone) and tests/test_notch_gpu.py."""
import numpy as np

import notch_spec as spec
from conftest import pkg
from oracle import softgnss_oracle as orc

CW_AMPLITUDE = 100          # LSB
CW_OFFSET_HZ = 180e3        # above IF
CW_PHASE = 0.3              # rad
THRESHOLD_DB = 8.0
WIDTH_HZ = 80e3
TAPS = 1025
PRESENT = (1, 3, 7, 11, 14, 19, 22, 31)
ABSENT = (5, 9)
MARGIN = 1.2

_CACHE = {}


def clean(ms):
    """Host copy of the default scene, long enough for `ms` tracking blocks behind the acquisition window."""
    synth = pkg("synth")
    s = orc.OracleSettings()
    key = ("clean", int(ms))
    if key not in _CACHE:
        _CACHE[key] = synth.generate(synth.Scene.default(), synth.record_length(s.samplesPerCode, ms))
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def jam(x, fs, f_hz, amplitude=CW_AMPLITUDE, phase=CW_PHASE):
    """x + rint(amplitude cos(2 pi f n / fs + phase)), clipped to +-127 as an ADC would."""
    n = np.arange(x.size, dtype=np.float64)
    cw = np.rint(amplitude * np.cos(2.0 * np.pi * f_hz * n / fs + phase)).astype(np.int64)
    return np.clip(x.astype(np.int64) + cw, -127, 127).astype(np.int8)


def jammed(ms):
    key = ("jammed", int(ms))
    if key not in _CACHE:
        s = orc.OracleSettings()
        _CACHE[key] = jam(clean(ms), s.samplingFreq, s.IF + CW_OFFSET_HZ)
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def contract_lines(x, s=None):
    """The contract's detect() on the oracle's probe statistics of the first 10 code periods."""
    s = s or orc.OracleSettings()
    f, pxx, _ = orc.probe_stats(s, x[:10 * s.samplesPerCode])
    return spec.detect(f, pxx, THRESHOLD_DB, WIDTH_HZ), f


def contract_mitigated(ms):
    """(filtered record, lines, taps, shift) by the contract alone."""
    key = ("mitigated", int(ms))
    if key not in _CACHE:
        s = orc.OracleSettings()
        x = jammed(ms)
        lines, _ = contract_lines(x, s)
        taps = spec.design(lines, s.samplingFreq, TAPS)
        y = spec.apply(x, taps, spec.DESIGN_SHIFT)
        y.setflags(write=False)
        _CACHE[key] = (y, lines, taps, spec.DESIGN_SHIFT)
    return _CACHE[key]
