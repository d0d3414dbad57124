"""The end-to-end scene of the front-end conditioning tests: an int16 (sc16) I/Q capture at zero IF that the fixed-gain chain
cannot read and the conditioning stage can.  Eight satellites in noise of sigma 12 per component (the level of
tests/iq_cases.py), then, as a front end would add them:

  * a constant DC per rail (DC_I, DC_Q, in units of the noise scale) - it follows the front end's gain,
  * a gain of GAIN_LO LSB per unit up to STEP_MS, GAIN_LO * STEP after it: the level rises once, mid-record, by 18 dB,
  * on top, at fixed level: pulses of a keyed carrier a quarter of the rate above the centre, PULSE_PEAK LSB, PULSE_LEN
    frames every PULSE_PERIOD frames (duty 2 %), each with its own phase.  A pulse is a whole number of carrier cycles, so
    it adds nothing to the mean of the block it falls in.

and the contracts' own two preparations of that file: tests/requant_spec.py at one fixed gain, or tests/cond_spec.py block by
block, then tests/iq_spec.py.  Deterministic and seeded; numpy and the oracle's C/A codes only.  Shared by
tests/test_cond_cases.py (CPU: the contracts plus the oracle alone), tests/test_cond_host.py and tests/test_cond_gpu.py.

Measured (tests/test_cond_cases.py prints them):
  fixed gain   rms 1810 LSB -> mult 27809 / 2^22 (-43.6 dB); 0.0005 % of the samples clipped, but the pulses stay in the
               record at 108 LSB against noise below 1 LSB: the oracle's search finds NONE of the eight, peak metric /
               acqThreshold = 0.90, 0.78, 0.62, 0.46, 0.59, 0.47, 0.64, 0.47 in the order of the PRNs below.
  conditioned  6.23 % of the frames blanked, no sample clipped, rms 11.6 LSB before and after the step; all eight found,
               peak metric / acqThreshold = 4.89, 4.37, 4.21, 5.99, 3.66, 6.42, 5.87, 5.70: the smallest is 3.66 >= 1.2."""
import numpy as np

import cond_spec as spec
import iq_cases
import iq_spec
import requant_spec
from oracle import softgnss_oracle as orc

SCENE = iq_cases.Scene("stepped_sc16", 0xC0D1, 4096000.0, 0.0, 63, (3, 6, 11, 14, 19, 22, 27, 30),
                       (1530.0, -3810.0, -2260.0, 4420.0, 3115.0, -1175.0, -640.0, 2290.0),
                       (1200.25, 6633.5, 5077.5, 2890.75, 333.75, 7811.0, 7400.0, 4150.25),
                       (6.5, 6.0, 5.5, 6.0, 5.5, 6.5, 6.0, 6.0), (0.3, -0.9, 1.9, 2.7, -2.2, 1.2, 0.8, -2.8))
MS = 304                    # the record: what 300 ms of tracking read
STEP_MS = 152               # the level steps here
GAIN_LO, STEP = 8.0, 8.0    # LSB per unit before the step; the factor of the step (18 dB)
DC_I, DC_Q = 9.0, -5.5      # units: 72 and -44 LSB before the step, 576 and -352 after it
PULSE_PEAK, PULSE_LEN, PULSE_PERIOD = 16000.0, 8, 400
MAX_CLIPPED = 1e-3          # the share of samples on +-127 a well prepared record stays below
# Settings of the stage, as Settings() has them
BLOCK_US, AGC_BLOCKS, BLANK_FACTOR, GUARD, TARGET_RMS = 100.0, 32.0, 4.0, 8, 12.0
LANES = 2
BLOCK = spec.block_frames(SCENE.fs_c, BLOCK_US)
BLANK_Q4 = spec.blank_q4_of(BLANK_FACTOR)
_CACHE = {}


def capture():
    """int16[MS * samples_per_code]: I0 Q0 I1 Q1 ... of the capture, read-only."""
    if "x" in _CACHE:
        return _CACHE["x"]
    sc = SCENE
    n = MS * sc.samples_per_code
    pairs = n // 2
    t = np.arange(pairs, dtype=np.float64) / sc.fs_c
    z = np.zeros(pairs, dtype=np.complex128)
    for i, prn in enumerate(sc.prns):
        code = orc.generate_ca_code(prn - 1)
        chips = (t - sc.code_start[i] / sc.fs) * iq_cases.CHIP_RATE * (1.0 + sc.doppler[i] / iq_cases.L1)
        period = np.floor(chips / 1023.0).astype(np.int64)
        bits = np.random.default_rng(sc.seed + 100 + prn).integers(0, 2, MS // 20 + 3) * 2 - 1
        chip = code[np.floor(chips).astype(np.int64) % 1023]
        z += sc.amplitude[i] * chip * bits[(period + 27) // 20] * np.exp(
            1j * (2.0 * np.pi * (sc.f_bb + sc.doppler[i]) * t + sc.phase[i]))
    z += iq_cases.NOISE_SIGMA * (np.random.default_rng(sc.seed).standard_normal(pairs)
                                 + 1j * np.random.default_rng(sc.seed + 1).standard_normal(pairs))
    z += DC_I + 1j * DC_Q
    step_at = STEP_MS * sc.samples_per_code // 2
    z *= np.where(np.arange(pairs) < step_at, GAIN_LO, GAIN_LO * STEP)
    f = np.arange(pairs)
    n_pulse = f // PULSE_PERIOD
    on = f % PULSE_PERIOD >= PULSE_PERIOD - PULSE_LEN - 100          # (the first one ends 100 frames before frame 400)
    on &= f % PULSE_PERIOD < PULSE_PERIOD - 100
    phase = np.random.default_rng(sc.seed + 7).uniform(0.0, 2.0 * np.pi, int(n_pulse[-1]) + 1)
    z += on * PULSE_PEAK * np.exp(1j * (0.5 * np.pi * f + phase[n_pulse]))
    assert max(np.abs(z.real).max(), np.abs(z.imag).max()) < 32000.0
    x = np.empty(n, dtype="<i2")
    x[0::2], x[1::2] = np.rint(z.real), np.rint(z.imag)
    x.setflags(write=False)
    _CACHE["x"] = x
    return x


def convert(y8, ms=None):
    """An int8 I/Q record through the converter's contract with the scene's filter; ms: only that many code periods of it
    (the filter is 63 taps long: all but the last few samples are those of the whole record's conversion)."""
    h, S = iq_cases.taps(SCENE)
    return iq_spec.convert(y8 if ms is None else y8[:ms * SCENE.samples_per_code], h, S)


def fixed_gain_record():
    """(int8 I/Q record, mult, shift): the capture through requant_spec at the one gain its statistics give."""
    if "fixed" not in _CACHE:
        x = capture()
        st = requant_spec.stats(x, x.dtype)
        mult, shift, _ = requant_spec.gain(st["n_finite"], st["sum_sq"], TARGET_RMS)
        _CACHE["fixed"] = (requant_spec.quantise(x, x.dtype, mult, shift), mult, shift)
    return _CACHE["fixed"]


def conditioned(x=None, lanes=LANES, block=BLOCK):
    """(statistics, plan, int8 record, blanked frames, clipped samples): x (default: the capture) through cond_spec at
    the stage's default settings."""
    key = "cond" if x is None else None
    if key and key in _CACHE:
        return _CACHE[key]
    x = capture() if x is None else x
    st = spec.block_stats(x, x.dtype, lanes, block, BLANK_Q4)
    plan = spec.plan(st, lanes, BLANK_Q4, TARGET_RMS, AGC_BLOCKS)
    y, blanked, clipped = spec.condition(x, x.dtype, lanes, block, plan, GUARD)
    out = (st, plan, y, blanked, clipped)
    if key:
        _CACHE[key] = out
    return out


def acquisition(which):
    """oracle.acquire on the first 11 code periods of the converted record: which = 'fixed' or 'conditioned'."""
    key = ("acq", which)
    if key not in _CACHE:
        y8 = fixed_gain_record()[0] if which == "fixed" else conditioned()[2]
        _CACHE[key] = orc.acquire(SCENE.oracle_settings(), convert(y8, 12)[:11 * SCENE.samples_per_code])
    return _CACHE[key]


REAL_FS, REAL_IF, REAL_SATS = 38192000.0, 9548000.0, 4     # the default rate: over 36 samples per chip, as trk3_kernel needs


def real_int16(ms):
    """int16[ms * 38192]: the scene's first REAL_SATS satellites as a REAL record at REAL_FS and REAL_IF, with a DC, the
    level step at half its length and no pulses - for the tracking of a real int16 record after conditioning."""
    key = ("real", int(ms))
    if key in _CACHE:
        return _CACHE[key]
    sc = SCENE
    n = int(ms) * int(REAL_FS / 1000.0)
    t = np.arange(n, dtype=np.float64) / REAL_FS
    v = np.zeros(n)
    for i, prn in enumerate(sc.prns[:REAL_SATS]):
        code = orc.generate_ca_code(prn - 1)
        chips = (t - sc.code_start[i] / REAL_FS) * iq_cases.CHIP_RATE * (1.0 + sc.doppler[i] / iq_cases.L1)
        period = np.floor(chips / 1023.0).astype(np.int64)
        bits = np.random.default_rng(sc.seed + 100 + prn).integers(0, 2, int(ms) // 20 + 3) * 2 - 1
        chip = code[np.floor(chips).astype(np.int64) % 1023]
        v += sc.amplitude[i] * chip * bits[(period + 27) // 20] * np.cos(
            2.0 * np.pi * (REAL_IF + sc.doppler[i]) * t + sc.phase[i])
    v += iq_cases.NOISE_SIGMA * np.random.default_rng(sc.seed + 2).standard_normal(n)
    v += DC_I
    v *= np.where(np.arange(n) < n // 2, GAIN_LO, GAIN_LO * STEP)
    x = np.rint(v).astype("<i2")
    x.setflags(write=False)
    _CACHE[key] = x
    return x
