"""The packed records of the unpacker's tests: scene 1 of tests/iq_cases.py, built from the float components BEFORE any
rounding (tests/requant_cases.py: components) and quantised to 1, 2 and 4 bits as a front end's ADC would, and the real
record the contract makes of that scene (iq_cases.contract_record) quantised to 2 bits; packed into files by
tests/unpack_spec.py: pack; and the contracts' own preparation of those files (unpack_spec, then iq_spec where I/Q) with
the oracle's acquisition on it, cached.  Deterministic and seeded; numpy and the oracle's C/A codes only.  Shared by
tests/test_unpack_host.py (CPU: the contracts plus the oracle alone) and tests/test_unpack_gpu.py.

The quantiser is mid-rise and uniform: k = clip(floor(v / step), -2^(b-1), 2^(b-1) - 1), level 2 k + 1.  1 bit: the sign
(v >= 0 gives +1).  2 bits: step 0.996 rms, the threshold at which a Gaussian input loses least.  4 bits: step 0.335 rms.
The rms is that of the first 11 code periods, so a shorter record is a prefix of a longer one."""
import numpy as np

import iq_cases
import iq_spec
import requant_cases
import unpack_spec as spec
from oracle import softgnss_oracle as orc

SCENE = iq_cases.SCENES[0]
STEP = {1: 1.0, 2: 0.996, 4: 0.335}      # in units of the rms (1 bit: any step gives the sign)
PEAK = spec.DEFAULT_PEAK
SKIP_SAMPLES = 2000                      # the non-zero skip of the end-to-end tests, in samples of the unpacked record
_CACHE = {}


class Case(object):
    """A packed file: how it is laid out (the arguments of the unpacker) and what it holds."""

    def __init__(self, name, bits, encoding, lsb_first, frame, first, iq):
        self.name, self.bits, self.encoding, self.lsb_first = name, bits, encoding, lsb_first
        self.frame, self.first, self.iq = frame, first, iq
        self.take = 2 if (iq and frame > 1) else 1
        self.flags = spec.LSB_FIRST if lsb_first else 0

    @property
    def table(self):
        return spec.table(self.bits, spec.ENCODINGS[self.encoding], PEAK)

    def file_bytes(self, samples):
        """Bytes of the file that `samples` samples of the unpacked record come from."""
        assert (samples * self.bits * self.frame) % (8 * self.take) == 0
        return samples * self.bits * self.frame // (8 * self.take)

    def settings(self, m, **kw):
        """The package's settings of the FILE."""
        s = SCENE.settings(m) if self.iq else m.Settings()
        if not self.iq:
            s.samplingFreq, s.IF, s.numberOfChannels = SCENE.fs, SCENE.IF, len(SCENE.prns)
        s.packedBits, s.packedEncoding, s.packedLsbFirst = self.bits, self.encoding, self.lsb_first
        s.packedFrame, s.packedFirst = self.frame, self.first
        for k, v in kw.items():
            setattr(s, k, v)
        return s


CASES = dict((c.name, c) for c in (
    Case("iq2", 2, "sign-magnitude", False, 1, 0, True),          # (a) 2-bit sign/magnitude I/Q, first field in the high bits
    Case("real2", 2, "sign-magnitude", False, 1, 0, False),       # (b) the real 2-bit record
    Case("iq1", 1, "offset-binary", True, 1, 0, True),            # (c) 1-bit offset-binary I/Q, first field in the low bits
    Case("ant4", 4, "twos-complement", False, 4, 2, True),        # (d) 4-bit two's-complement, two antennas: the second
))


def quantise(v, bits, rms):
    """Levels 2 k + 1 of the mid-rise quantiser with step STEP[bits] rms."""
    k = np.floor(np.asarray(v, dtype=np.float64) / (STEP[bits] * rms)).astype(np.int64)
    return 2 * np.clip(k, -(1 << (bits - 1)), (1 << (bits - 1)) - 1) + 1


def source(case, ms):
    """float64: what the front end of the case samples, ms code periods of the unpacked record."""
    if case.iq:
        return requant_cases.components(ms)
    return iq_cases.contract_record(SCENE, ms).astype(np.float64)


def levels(case, ms):
    key = ("levels", case.name, int(ms))
    if key not in _CACHE:
        head = source(case, 11)
        lv = quantise(source(case, ms), case.bits, float(np.sqrt(np.mean(head * head))))
        lv.setflags(write=False)
        _CACHE[key] = lv
    return _CACHE[key]


def file_of(case, ms):
    """uint8: the packed file of the case, read-only.  With a frame of four fields (two antennas, I/Q each) the first
    antenna holds other noise, the second the scene."""
    key = ("file", case.name, int(ms))
    if key not in _CACHE:
        inv = spec.code_of_level(case.bits, spec.ENCODINGS[case.encoding])
        c = inv[(levels(case, ms) + (1 << case.bits) - 1) // 2]
        if case.frame > 1:
            assert case.frame == 4 and case.first == 2 and case.take == 2
            fields = np.random.default_rng(SCENE.seed + 77).integers(0, 1 << case.bits, (c.size // 2, 4))
            fields[:, 2:] = c.reshape(-1, 2)
            c = fields.reshape(-1)
        b = spec.pack(c, case.bits, case.flags)
        b.setflags(write=False)
        _CACHE[key] = b
    return _CACHE[key]


def unpacked(case, b):
    """The contract's int8 record of the file bytes b."""
    return spec.unpack(b, case.bits, case.table, case.flags, case.frame, case.first, case.take)


def prepared(case, b):
    """The contracts' prepared record of the file bytes b: unpacked, then converted where the case is I/Q."""
    y = unpacked(case, b)
    if case.iq:
        h, S = iq_cases.taps(SCENE)
        y = iq_spec.convert(y, h, S)
    return y


def contract_record(case, ms):
    key = ("prepared", case.name, int(ms))
    if key not in _CACHE:
        y = prepared(case, file_of(case, ms))
        y.setflags(write=False)
        _CACHE[key] = y
    return _CACHE[key]


def contract_acquisition(case, ms=11):
    """oracle.acquire on the first 11 code periods of the contracts' record."""
    key = ("acq", case.name, int(ms))
    if key not in _CACHE:
        _CACHE[key] = orc.acquire(SCENE.oracle_settings(), contract_record(case, ms)[:11 * SCENE.samples_per_code])
    return _CACHE[key]
