"""The two end-to-end scenes of the chain tests - the chains the resampler was written for, a low-rate capture brought up to
the rate the speculative tracking kernel needs - and the composed contract's preparation of them (tests/chain_cases.py):

  A  scene a of tests/decim_cases.py (I/Q at 16.368 Msps, the carrier 3.2 MHz off centre) quantised to 2 bits as a front end's
     ADC would and packed sign/magnitude; read through packedBits = 2, iqRecord, decimation = 4, resampleUp = 5: a real record
     at 40.92 Msps.
  B  the four satellites of scene a of tests/resamp_cases.py as a real int16 record at 4.096 Msps with the DC, the level step
     (18 dB, mid-record) and the pulses (a keyed carrier at a quarter of the rate, duty 2 %) of tests/cond_cases.py; read
     through frontEndConditioning, resampleUp = 10: a real record at 40.96 Msps.

Deterministic and seeded; numpy and the oracle's C/A codes only.  Shared by tests/test_chain_host.py (CPU: the contracts plus
the oracle alone) and tests/test_chain_gpu.py."""
import numpy as np

import chain_cases as cases
import cond_cases
import decim_cases as dc
import resamp_cases
import unpack_cases
import unpack_spec
from oracle import softgnss_oracle as orc

MARGIN, ABSENT_MAX = dc.MARGIN, dc.ABSENT_MAX
TRK_MS = resamp_cases.TRK_MS            # 200 code periods tracked end to end
ACQ_MS = 12
SKIP_UNITS = 1237                       # the end-to-end skip, in the chain's smallest legal skipNumberOfBytes
_CACHE = {}


class Scene(object):
    def __init__(self, name, source, chain, make):
        self.name, self.source, self.chain, self._make = name, source, chain, make
        self.prns = source.prns

    def file_of(self, ms):
        key = (self.name, int(ms))
        if key not in _CACHE:
            b = self._make(self.source, int(ms))
            b.setflags(write=False)
            _CACHE[key] = b
        return _CACHE[key]

    @property
    def skip_bytes(self):
        return SKIP_UNITS * cases.skip_unit(self.chain)

    def skip_out(self, skip_bytes):
        return cases.prepared_skip(self.chain, skip_bytes)

    def settings(self, m, **kw):
        return self.chain.settings(m, numberOfChannels=len(self.prns), **kw)

    def oracle_settings(self, **kw):
        p = cases.prepared_settings(self.chain)
        return orc.OracleSettings(samplingFreq=p["samplingFreq"], IF=p["IF"], numberOfChannels=len(self.prns), **kw)


def _packed_iq(source, ms):
    """decim_cases' int8 I/Q record through the 2-bit quantiser of tests/unpack_cases.py (step 0.996 of the rms of the first
    11 code periods, so that a shorter file is a prefix of a longer one), packed sign/magnitude, first field in the high bits."""
    x = dc.record(source, ms).astype(np.float64)
    head = x[:11 * source.frames_per_ms * 2]
    lv = unpack_cases.quantise(x, 2, float(np.sqrt(np.mean(head * head))))
    code = unpack_spec.code_of_level(2, unpack_spec.SIGN_MAGNITUDE)[(lv + 3) // 2]
    return unpack_spec.pack(code, 2)


def _stepped_int16(source, ms):
    """A real int16 record: the scene's satellites in noise of sigma 12, then a DC, the gain of cond_cases with its step at
    half the record, and on top its pulses at fixed level."""
    cc = cond_cases
    n = ms * source.frames_per_ms
    t = np.arange(n, dtype=np.float64) / source.fs
    v = dc.NOISE_SIGMA * np.random.default_rng(source.seed).standard_normal(n)
    for i, prn in enumerate(source.prns):
        code = orc.generate_ca_code(prn - 1)
        bits = np.random.default_rng(source.seed + 100 + prn).integers(0, 2, ms // 20 + 3) * 2 - 1
        chips = (t - source.code_start_s[i]) * dc.CHIP_RATE * (1.0 + source.doppler[i] / dc.L1)
        period = np.floor(chips / 1023.0).astype(np.int64)
        chip = code[np.floor(chips).astype(np.int64) % 1023]
        v += source.amplitude[i] * chip * bits[(period + 27) // 20] * np.cos(
            2.0 * np.pi * (source.f0 + source.doppler[i]) * t + source.phase[i])
    v += cc.DC_I
    step_at = (TRK_MS + 4) * source.frames_per_ms // 2   # (a fixed instant: a shorter file is a prefix of a longer one)
    v *= np.where(np.arange(n) < step_at, cc.GAIN_LO, cc.GAIN_LO * cc.STEP)
    f = np.arange(n)
    k = f // cc.PULSE_PERIOD
    on = (f % cc.PULSE_PERIOD >= cc.PULSE_PERIOD - cc.PULSE_LEN - 100) & (f % cc.PULSE_PERIOD < cc.PULSE_PERIOD - 100)
    phase = np.random.default_rng(source.seed + 7).uniform(0.0, 2.0 * np.pi, (TRK_MS + 4) * source.frames_per_ms
                                                           // cc.PULSE_PERIOD + 1)
    v += on * cc.PULSE_PEAK * np.cos(0.5 * np.pi * f + phase[k])
    assert np.abs(v).max() < 32000.0
    return np.rint(v).astype("<i2").view(np.uint8)


# (the noise seeds are those of the scenes the two come from; they were kept after the CPU showed that with them the oracle
# alone, on the composed contract's records, finds each scene's four satellites at least MARGIN above the threshold and stays
# at or below ABSENT_MAX on all 28 absent PRNs, in both windows the end-to-end tests acquire in - at the start and behind
# SKIP_UNITS units: tests/test_chain_host.py asserts it)
SOURCE_A = dc.Scene("iq_16368_2bit", 0x1DEC1, 2, 16368000.0, 3200000.0, dc.SCENE_A.prns, dc.SCENE_A.doppler,
                    dc.SCENE_A.code_start_s, dc.SCENE_A.amplitude, dc.SCENE_A.phase)
_RA = resamp_cases.SCENE_A
SOURCE_B = dc.Scene("real_4096_stepped", 0x5A3FB, 1, _RA.fs, _RA.f0, _RA.prns, _RA.doppler, _RA.code_start_s, _RA.amplitude,
                    _RA.phase)
SCENE_A = Scene("packed2_iq_d4_r5", SOURCE_A,
                cases.Chain(first="packed", bits=2, iq=True, D=4, resamp=(5, 1), fs=SOURCE_A.fs, f0=SOURCE_A.f0), _packed_iq)
SCENE_B = Scene("cond_int16_r10", SOURCE_B,
                cases.Chain(first="cond", dtype="int16", resamp=(10, 1), fs=SOURCE_B.fs, f0=SOURCE_B.f0), _stepped_int16)
SCENES = {"A": SCENE_A, "B": SCENE_B}


def prepared(scene, ms):
    """chain_cases.prepare of the whole of file_of(ms), as postProcessing prepares it (offset 0: a skip only picks the
    window that is searched)."""
    key = ("prepared", scene.name, int(ms))
    if key not in _CACHE:
        b = scene.file_of(ms)
        out = cases.prepare(b, scene.chain, 0, cases.prepared_length(scene.chain, b.size))
        out["record"].setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def contract_acquisition(scene, skip_bytes=0):
    """oracle.acquire on 11 code periods of the composed contract's record, from the sample byte skip_bytes becomes."""
    key = ("acq", scene.name, int(skip_bytes))
    if key not in _CACHE:
        o = scene.oracle_settings()
        skip = scene.skip_out(skip_bytes)
        window = prepared(scene, ACQ_MS)["record"][skip:skip + 11 * o.samplesPerCode]
        assert window.size == 11 * o.samplesPerCode
        _CACHE[key] = orc.acquire(o, window)
    return _CACHE[key]
