"""The two scenes of the I/Q front-stage tests: interleaved int8 I/Q records at or near zero IF, four satellites each, and
the contract's own conversion of them (tests/iq_spec.py).  Deterministic and seeded; numpy and the oracle's C/A codes only.
Shared by tests/test_iq_host.py (CPU: the contract plus the oracle alone) and tests/test_iq_gpu.py."""
import numpy as np

import iq_spec as spec
from oracle import softgnss_oracle as orc

L1 = 1575.42e6
CHIP_RATE = 1023000.0
MARGIN = 1.2                # detected peaks stand at least this far above acqThreshold
CARR_TOL_HZ = 100.0         # carrFreq against the truth
PHASE_TOL = 2.0             # code phase against the truth, samples of the converted record
NOISE_SIGMA = 12.0          # LSB per component


class Scene(object):
    """fs_c: complex rate; f_bb: baseband offset of the L1 carrier; per satellite a PRN (1-based), a Doppler (Hz), the
    instant its code starts (in samples of the CONVERTED record, i.e. bytes of the file), an amplitude (LSB) and a
    carrier phase (rad)."""

    def __init__(self, name, seed, fs_c, f_bb, taps, prns, doppler, code_start, amplitude, phase):
        self.name, self.seed, self.fs_c, self.f_bb, self.taps = name, seed, float(fs_c), float(f_bb), int(taps)
        self.prns, self.doppler, self.code_start = tuple(prns), tuple(doppler), tuple(code_start)
        self.amplitude, self.phase = tuple(amplitude), tuple(phase)
        self.fs, self.IF = spec.real_equivalent(self.fs_c, self.f_bb)

    @property
    def samples_per_code(self):
        return int(round(self.fs / 1000.0))

    def true_carrier(self, i):
        return self.IF + self.doppler[i]

    def oracle_settings(self, **kw):
        """The oracle's settings of the CONVERTED record."""
        return orc.OracleSettings(samplingFreq=self.fs, IF=self.IF, numberOfChannels=len(self.prns), **kw)

    def settings(self, m, **kw):
        """The package's settings of the I/Q FILE: the complex rate, the baseband offset, iqRecord set."""
        s = m.Settings()
        s.samplingFreq, s.IF, s.iqRecord, s.iqTaps = self.fs_c, self.f_bb, True, self.taps
        s.numberOfChannels = len(self.prns)
        for k, v in kw.items():
            setattr(s, k, v)
        return s


SCENES = (
    Scene("zero_if_4096", 0x1A51, 4096000.0, 0.0, 63, (3, 11, 19, 27), (1530.0, -2260.0, 3115.0, -640.0),
          (1200.25, 5077.5, 333.75, 7400.0), (6.0, 5.0, 5.5, 6.0), (0.3, 1.9, -2.2, 0.8)),
    Scene("offset_5000", 0x1A52, 5000000.0, 20000.0, 31, (2, 8, 14, 30), (-3370.0, 880.0, 2405.0, -1515.0),
          (9100.5, 2500.25, 6020.0, 415.75), (6.0, 5.5, 5.0, 6.0), (-1.1, 0.4, 2.6, -0.2)),
)
_CACHE = {}


def iq_record(scene, ms):
    """int8[2 * pairs] interleaved I, Q of `ms` code periods of the CONVERTED record (ms * samples_per_code bytes)."""
    key = ("iq", scene.name, int(ms))
    if key in _CACHE:
        return _CACHE[key]
    n_bytes = int(ms) * scene.samples_per_code
    assert n_bytes % 2 == 0
    pairs = n_bytes // 2
    t = np.arange(pairs, dtype=np.float64) / scene.fs_c
    z = np.zeros(pairs, dtype=np.complex128)
    for i, prn in enumerate(scene.prns):
        code = orc.generate_ca_code(prn - 1)
        t0 = scene.code_start[i] / scene.fs
        chips = (t - t0) * CHIP_RATE * (1.0 + scene.doppler[i] / L1)
        period = np.floor(chips / 1023.0).astype(np.int64)
        # navigation bits of 20 code periods; the first edge lies behind the 11 ms that acquisition reads
        bits = np.random.default_rng(scene.seed + 100 + prn).integers(0, 2, int(ms) // 20 + 3) * 2 - 1
        data = bits[(period + 27) // 20]
        chip = code[np.floor(chips).astype(np.int64) % 1023]
        z += scene.amplitude[i] * chip * data * np.exp(1j * (2.0 * np.pi * (scene.f_bb + scene.doppler[i]) * t + scene.phase[i]))
    # one generator per component: a shorter record is a prefix of a longer one
    z += NOISE_SIGMA * (np.random.default_rng(scene.seed).standard_normal(pairs)
                        + 1j * np.random.default_rng(scene.seed + 1).standard_normal(pairs))
    b = np.empty(n_bytes, dtype=np.int8)
    b[0::2] = np.clip(np.rint(z.real), -128, 127)
    b[1::2] = np.clip(np.rint(z.imag), -128, 127)
    b.setflags(write=False)
    _CACHE[key] = b
    return b


def taps(scene):
    return spec.design(scene.taps)


def contract_record(scene, ms):
    """The contract's conversion of iq_record(scene, ms)."""
    key = ("real", scene.name, int(ms))
    if key not in _CACHE:
        h, S = taps(scene)
        y = spec.convert(iq_record(scene, ms), h, S)
        y.setflags(write=False)
        _CACHE[key] = y
    return _CACHE[key]


def contract_acquisition(scene, ms=11):
    """oracle.acquire on the first 11 code periods of the contract's record."""
    key = ("acq", scene.name, int(ms))
    if key not in _CACHE:
        n = scene.samples_per_code
        _CACHE[key] = orc.acquire(scene.oracle_settings(), contract_record(scene, ms)[:11 * n])
    return _CACHE[key]
