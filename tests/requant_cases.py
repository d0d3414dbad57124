"""Scene 1 of tests/iq_cases.py as a wide capture: the same four satellites and the same noise, built anew from the float
values BEFORE any rounding and written as interleaved int16 (sc16, rms near 500 LSB) and float32 (fc32, rms near 2^-11)
I/Q; and the contracts' own preparation of those files (tests/requant_spec.py, then tests/iq_spec.py).  Deterministic and
seeded; numpy and the oracle's C/A codes only.  Shared by tests/test_requant_host.py (CPU: the contracts plus the oracle
alone) and tests/test_requant_gpu.py."""
import numpy as np

import iq_cases
import iq_spec
import requant_spec as spec
from oracle import softgnss_oracle as orc

SCENE = iq_cases.SCENES[0]
# the scene's components have an rms of about 14.4 (noise of sigma 12 plus four satellites of 5 - 6 LSB)
SCALE = {"int16": 35.0, "float32": 3.4e-5}       # -> rms about 504 LSB; about 4.9e-4 = 1.003 * 2^-11
TARGET_RMS = spec.DEFAULT_TARGET_RMS
_CACHE = {}


def components(ms):
    """float64[ms * samples_per_code]: I0 Q0 I1 Q1 ... of scene 1 before rounding, as tests/iq_cases.py: iq_record builds
    them (one noise generator per component, so a shorter record is a prefix of a longer one)."""
    key = ("z", int(ms))
    if key in _CACHE:
        return _CACHE[key]
    sc = SCENE
    n = int(ms) * sc.samples_per_code
    assert n % 2 == 0
    pairs = n // 2
    t = np.arange(pairs, dtype=np.float64) / sc.fs_c
    z = np.zeros(pairs, dtype=np.complex128)
    for i, prn in enumerate(sc.prns):
        code = orc.generate_ca_code(prn - 1)
        chips = (t - sc.code_start[i] / sc.fs) * iq_cases.CHIP_RATE * (1.0 + sc.doppler[i] / iq_cases.L1)
        period = np.floor(chips / 1023.0).astype(np.int64)
        bits = np.random.default_rng(sc.seed + 100 + prn).integers(0, 2, int(ms) // 20 + 3) * 2 - 1
        chip = code[np.floor(chips).astype(np.int64) % 1023]
        z += sc.amplitude[i] * chip * bits[(period + 27) // 20] * np.exp(
            1j * (2.0 * np.pi * (sc.f_bb + sc.doppler[i]) * t + sc.phase[i]))
    z += iq_cases.NOISE_SIGMA * (np.random.default_rng(sc.seed).standard_normal(pairs)
                                 + 1j * np.random.default_rng(sc.seed + 1).standard_normal(pairs))
    out = np.empty(n, dtype=np.float64)
    out[0::2], out[1::2] = z.real, z.imag
    out.setflags(write=False)
    _CACHE[key] = out
    return out


def wide_record(dtype, ms):
    """The file's elements: int16 (rounded half to even, no value near the rails) or float32, read-only."""
    name = np.dtype(dtype).name
    key = ("wide", name, int(ms))
    if key not in _CACHE:
        v = components(ms) * SCALE[name]
        x = np.rint(v).astype("<i2") if name == "int16" else v.astype("<f4")
        assert np.abs(v).max() < 32000.0
        x.setflags(write=False)
        _CACHE[key] = x
    return _CACHE[key]


def contract_gain(x, target_rms=TARGET_RMS):
    """(statistics, mult, shift, scale) of the contract for the whole of x."""
    st = spec.stats(x, x.dtype)
    return (st,) + spec.gain(st["n_finite"], st["sum_sq"], target_rms)


def contract_record(x, mult, shift, scale):
    """x through the requantiser's contract at this gain, then through the converter's with the scene's filter."""
    h, S = iq_cases.taps(SCENE)
    return iq_spec.convert(spec.quantise(x, x.dtype, mult, shift, scale), h, S)


def contract_acquisition(dtype, ms=11):
    """oracle.acquire on the first 11 code periods of the contracts' record of wide_record(dtype, ms)."""
    key = ("acq", np.dtype(dtype).name, int(ms))
    if key not in _CACHE:
        x = wide_record(dtype, ms)
        _, mult, shift, scale = contract_gain(x)
        y = contract_record(x, mult, shift, scale)
        _CACHE[key] = orc.acquire(SCENE.oracle_settings(), y[:11 * SCENE.samples_per_code])
    return _CACHE[key]
