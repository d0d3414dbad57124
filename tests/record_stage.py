"""What the GPU tests of the two record-conditioning stages share (tests/test_notch_gpu.py, tests/test_iq_gpu.py): the
full-scale input bytes, and the bar the tracking on a prepared record is held to."""
import numpy as np

from test_gpu_parity import TRK_TOL      # max |delta| of the correlator series over max(1, RMS |P|) per channel


def full_scale(rng, n):
    """n random int8 samples over the whole range, both rails among them at known places."""
    x = rng.integers(-128, 128, n).astype(np.int8)
    x[::97] = -128
    x[5::101] = 127
    return x


def same_tracking(t, series, channels, ms):
    """A TrackingResult against the oracle's stacked series: every block boundary equal, the six correlator series of
    every channel within TRK_TOL of the oracle's."""
    assert t.series.shape == series.shape == (channels, 13, ms)
    assert np.array_equal(t.series[:, 0], series[:, 0])                 # absoluteSample: every block boundary
    worst = 0.0
    for ch in range(channels):
        scale = max(1.0, float(np.sqrt(np.mean(series[ch, 3] ** 2 + series[ch, 7] ** 2))))
        worst = max(worst, float(np.max(np.abs(t.series[ch, 3:9] - series[ch, 3:9]))) / scale)
    assert worst < TRK_TOL, worst
