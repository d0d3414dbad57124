"""Full-scale IF records for the tracking kernels' fixed-point limits (tests/test_full_scale_gpu.py, checked on the CPU
by tests/test_full_scale_records.py).

Every typed tracking kernel sums samples in fixed point and has a range it must stay inside; the synthetic scene's samples
are small and never get near it.  These records do: noiseless ones whose every sample lines up with the replica, 1-bit
(hard-clipped) ones, and the default scene overdriven into the type's limits (an AGC gone wrong).  All of them are pure
numpy functions of their arguments."""
import numpy as np

# sgx_trk3.hip: a unit's 2 048 bytes must add up to less than 2^17 in magnitude (mean |x| 64) for the speculative kernel
TRK3_WINDOW = 2048
TRK3_BOUND = 131072
# the host scan (sgx_trk.hip: if_mag_bound) looks at 17 consecutive 128-byte blocks, a superset of any kernel window
HOST_WINDOW = 17 * 128
# a record "below" / "above" the bound is so by at least this fraction of it
MARGIN = 0.05

# noiseless int8 amplitudes: below the bound on the host's wider window, and above it on the kernel's exact one
INT8_BELOW = (50, 80)
INT8_ABOVE = (106, 127)

LIMITS = {"int8": (-128, 127), "uint8": (0, 255), "int16": (-32768, 32767)}

# the low-rate front end of test_other_front_ends_against_oracle: 5.3 samples per chip (the per-sample kernels)
LOW_RATE = (5456000.0, 1364000.0)


def clean_record(m, s, amp, n_ms, prn=5, doppler=1250.0, start=7000):
    """A NOISELESS one-satellite record: round(amp * chip * cos(carrier)) - every sample lines up with the replica."""
    n = s.samplesPerCode
    N = (n_ms + 2) * (n + 2)
    t = np.arange(N, dtype=np.float64)
    code = np.asarray(s.generateCAcode(prn - 1))
    chip = code[(np.floor((t - start) * (s.codeFreqBasis / s.samplingFreq)).astype(np.int64)) % 1023]
    x = np.rint(amp * chip * np.cos(2 * np.pi * ((s.IF + doppler) / s.samplingFreq) * t + 0.3))
    return x.astype(np.int64)


def clean_channel(s, prn=5, doppler=1250.0, start=7000):
    """The (PRN, acquiredFreq, first sample) that clean_record / clipped_record were made with."""
    return prn, s.IF + doppler, start


def clipped_record(m, s, dtype, n_ms, **kw):
    """A 1-bit record at full scale: the type's largest value where chip * cos >= 0, its smallest elsewhere."""
    lo, hi = LIMITS[dtype]
    x = clean_record(m, s, 1000, n_ms, **kw)
    return np.where(x >= 0, hi, lo).astype(dtype)


def as_type(x, dtype):
    """Signed integers (int64) as a record of `dtype`: clipped to the type's range; uint8 offset-binary (x + 128)."""
    if dtype == "uint8":
        return np.clip(x + 128, 0, 255).astype(np.uint8)
    lo, hi = LIMITS[dtype]
    return np.clip(x, lo, hi).astype(dtype)


def saturated_record(m, s, dtype, n_ms, gain=None):
    """The default scene (8 satellites and noise of sigma ~20) times a large gain, clipped to the type's range: most samples
    sit at a rail (an overdriven AGC).  Channels: saturated_channels."""
    sc = m.synth.Scene.default(s.samplingFreq, s.IF)
    x = m.synth.generate(sc, m.synth.record_length(s.samplesPerCode, n_ms)).astype(np.int64)
    if gain is None:
        gain = 4096 if dtype == "int16" else 16
    return as_type(x * gain, dtype)


def saturated_channels(s):
    """PRN 1 and PRN 14 of the default scene (synth.Scene.default): (PRN, acquiredFreq, first sample)."""
    return [(1, s.IF + 1250.0, 12345), (14, s.IF + 2900.0, 777)]


def float_record(x, dtype, exp=20):
    """x (integers, or any float64 values) times 2^exp, as float32 / float64: exact, so the record is x scaled."""
    return (np.asarray(x, dtype=np.float64) * 2.0 ** exp).astype(dtype)


def unrounded_record(m, s, amp, n_ms, prn=5, doppler=1250.0, start=7000):
    """clean_record before its rounding: floats that no power of two turns into integers of 16 bits."""
    n = s.samplesPerCode
    N = (n_ms + 2) * (n + 2)
    t = np.arange(N, dtype=np.float64)
    code = np.asarray(s.generateCAcode(prn - 1))
    chip = code[(np.floor((t - start) * (s.codeFreqBasis / s.samplingFreq)).astype(np.int64)) % 1023]
    return amp * chip * np.cos(2 * np.pi * ((s.IF + doppler) / s.samplingFreq) * t + 0.3)


def window_mag_max(x, width):
    """The largest sum of |x| over any `width` consecutive samples (int8 bytes: magnitudes as the kernels read them)."""
    a = np.abs(np.asarray(x, dtype=np.int64))
    c = np.concatenate([[0], np.cumsum(a)])
    return int((c[width:] - c[:-width]).max())


def int8_records(m, s, n_ms):
    """name -> (int8 record, above the bound?) for every int8 record of the suite at the default front end."""
    out = {}
    for a in INT8_BELOW:
        out["clean%d" % a] = (clean_record(m, s, a, n_ms).astype(np.int8), False)
    for a in INT8_ABOVE:
        out["clean%d" % a] = (clean_record(m, s, a, n_ms).astype(np.int8), True)
    out["clipped"] = (clipped_record(m, s, "int8", n_ms), True)
    out["saturated"] = (saturated_record(m, s, "int8", n_ms), True)
    return out
