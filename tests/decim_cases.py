"""The two scenes of the decimation tests and the contracts' own preparation of them (tests/decim_spec.py, and
tests/iq_spec.py behind it for the I/Q scene): (a) a 16.368 Msps complex capture whose centre lies 3.2 MHz below L1,
decimated by 4 through 63 and 127 taps and converted to real IF; (b) the default real front end, 38.192 Msps with the IF at
9.548 MHz, decimated by 5 (upright) and by 3 (inverted).  Four satellites each.  Deterministic and seeded; numpy and the
oracle's C/A codes only.  Shared by tests/test_decim_host.py (CPU: the contracts plus the oracle alone) and
tests/test_decim_gpu.py."""
import numpy as np

import decim_spec as spec
import iq_spec
from oracle import softgnss_oracle as orc

L1 = 1575.42e6
CHIP_RATE = 1023000.0
MARGIN = 1.2                # detected peaks stand at least this far above acqThreshold
CARR_TOL_HZ = 100.0         # carrFreq against the truth
PHASE_TOL = 2.0             # code phase against the truth, samples of the prepared record
ABSENT_MAX = 2.2            # the oracle's peak metric of every PRN the scene does not hold, against acqThreshold 2.5
NOISE_SIGMA = 12.0          # LSB per component
ACQ_MS = 12                 # code periods of the records the CPU tests look at
TRK_MS = 1000               # code periods tracked end to end
SKIP_GROUPS = 1237          # the end-to-end skip: that many groups of D input frames
IQ_TAPS = 63                # Settings.iqTaps


class Scene(object):
    """lanes 1: a real record at rate fs with the carrier at f0; lanes 2: interleaved I/Q at the complex rate fs with the
    carrier f0 off the centre.  Per satellite a PRN (1-based), a Doppler (Hz), the instant its code starts (s), an
    amplitude (LSB) and a carrier phase (rad)."""

    def __init__(self, name, seed, lanes, fs, f0, prns, doppler, code_start_s, amplitude, phase):
        self.name, self.seed, self.lanes, self.fs, self.f0 = name, seed, int(lanes), float(fs), float(f0)
        self.prns, self.doppler, self.code_start_s = tuple(prns), tuple(doppler), tuple(code_start_s)
        self.amplitude, self.phase = tuple(amplitude), tuple(phase)

    @property
    def frames_per_ms(self):
        return int(round(self.fs / 1000.0))


class Case(object):
    """A scene, a factor and a filter length: what Settings.decimation, decimTaps and the defaults make of the file."""

    def __init__(self, scene, D, L):
        self.scene, self.D, self.L, self.lanes = scene, int(D), int(L), scene.lanes
        self.taps, self.shift, fs_out, f_out, inverted = spec.design(scene.fs, scene.f0, spec.DEFAULT_BANDWIDTH, scene.lanes,
                                                                     D, L)
        self.design_out = (fs_out, f_out, inverted)
        self.gain = spec.default_gain(scene.fs, spec.DEFAULT_BANDWIDTH, scene.lanes)

    def prepared_rate(self):
        """(samplingFreq, IF) of the prepared record: the decimated one, for I/Q its real equivalent."""
        fs_out, f_out, _ = self.design_out
        return iq_spec.real_equivalent(fs_out, f_out) if self.lanes == 2 else (fs_out, f_out)

    def true_carrier(self, i):
        """Where satellite i's carrier lies in the prepared record: an inverted band flips the sign of the Doppler."""
        _, if_p = self.prepared_rate()
        return if_p + (-1.0 if self.design_out[2] else 1.0) * self.scene.doppler[i]

    def true_phase(self, i):
        """Satellite i's code phase in samples of the prepared record."""
        fs_p, _ = self.prepared_rate()
        return self.scene.code_start_s[i] * fs_p

    def amplitude_out(self, i):
        """The amplitude of satellite i's carrier behind the stage's gain (the part of its code the band passes aside)."""
        return self.scene.amplitude[i] * self.gain

    def settings(self, m, **kw):
        """The package's settings of the FILE."""
        s = m.Settings()
        s.samplingFreq, s.IF, s.iqRecord, s.iqTaps = self.scene.fs, self.scene.f0, self.lanes == 2, IQ_TAPS
        s.decimation, s.decimTaps = self.D, self.L
        s.numberOfChannels = len(self.scene.prns)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def oracle_settings(self, **kw):
        fs_p, if_p = self.prepared_rate()
        return orc.OracleSettings(samplingFreq=fs_p, IF=if_p, numberOfChannels=len(self.scene.prns), **kw)


SCENE_A = Scene("iq_16368", 0x1DEC1, 2, 16368000.0, 3200000.0, (3, 11, 19, 27), (1530.0, -2260.0, 3115.0, -640.0),
                (146.65e-6, 620.4e-6, 40.78e-6, 904.2e-6), (6.0, 5.0, 5.5, 6.0), (0.3, 1.9, -2.2, 0.8))
# (the noise seeds were picked on the CPU so that the oracle alone, on the contracts' records, stays at or below ABSENT_MAX on
# all 28 PRNs that are absent, in every case and in both windows the end-to-end tests acquire in - at the start and behind
# SKIP_GROUPS groups: tests/test_decim_host.py asserts it)
SCENE_B = Scene("real_38192", 0x1DECF, 1, 38192000.0, 9548000.0, (3, 11, 19, 27), (-3370.0, 880.0, 2405.0, -1515.0),
                (311.9e-6, 85.7e-6, 726.3e-6, 533.1e-6), (6.0, 5.5, 5.0, 6.0), (-1.1, 0.4, 2.6, -0.2))
CASES = {
    "iq_d4_63": Case(SCENE_A, 4, 63),
    "iq_d4_127": Case(SCENE_A, 4, 127),
    "real_d5": Case(SCENE_B, 5, 127),
    "real_d3": Case(SCENE_B, 3, 127),
}
_CACHE = {}


def record(scene, ms):
    """int8 bytes of `ms` code periods of the scene's file: ms * frames_per_ms frames of `lanes` bytes."""
    key = ("file", scene.name, int(ms))
    if key in _CACHE:
        return _CACHE[key]
    frames = int(ms) * scene.frames_per_ms
    # one generator per component: a shorter record is a prefix of a longer one
    noise = [NOISE_SIGMA * np.random.default_rng(scene.seed + c).standard_normal(frames) for c in range(scene.lanes)]
    z = noise[0] + 1j * noise[1] if scene.lanes == 2 else noise[0]
    step = 4 * 1024 * 1024                              # (in pieces: the whole second would take gigabytes of temporaries)
    for i, prn in enumerate(scene.prns):
        code = orc.generate_ca_code(prn - 1)
        bits = np.random.default_rng(scene.seed + 100 + prn).integers(0, 2, int(ms) // 20 + 3) * 2 - 1
        for lo in range(0, frames, step):
            t = np.arange(lo, min(frames, lo + step), dtype=np.float64) / scene.fs
            chips = (t - scene.code_start_s[i]) * CHIP_RATE * (1.0 + scene.doppler[i] / L1)
            period = np.floor(chips / 1023.0).astype(np.int64)
            # navigation bits of 20 code periods; the first edge lies behind the 11 ms that acquisition reads
            data = bits[(period + 27) // 20]
            chip = code[np.floor(chips).astype(np.int64) % 1023]
            arg = 2.0 * np.pi * (scene.f0 + scene.doppler[i]) * t + scene.phase[i]
            carrier = np.exp(1j * arg) if scene.lanes == 2 else np.cos(arg)
            z[lo:lo + t.size] += scene.amplitude[i] * chip * data * carrier
    b = np.empty(frames * scene.lanes, dtype=np.int8)
    if scene.lanes == 2:
        b[0::2] = np.clip(np.rint(z.real), -128, 127)
        b[1::2] = np.clip(np.rint(z.imag), -128, 127)
    else:
        b[:] = np.clip(np.rint(z), -128, 127)
    b.setflags(write=False)
    _CACHE[key] = b
    return b


def file_of(case, ms):
    return record(case.scene, ms)


def prepared_of(case, decimated):
    """The prepared record the contracts make of a decimated one: itself, or for I/Q its conversion to real IF."""
    if case.lanes == 1:
        return decimated
    h, S = iq_spec.design(IQ_TAPS)
    return iq_spec.convert(decimated, h, S)


def prepared(case, ms):
    """The contracts' prepared record of file_of(case, ms)."""
    key = ("prepared", case.scene.name, case.D, case.L, int(ms))
    if key not in _CACHE:
        y = prepared_of(case, spec.decimate(file_of(case, ms), case.taps, case.shift, case.lanes, case.D)[0])
        y.setflags(write=False)
        _CACHE[key] = y
    return _CACHE[key]


def _decimated_whole(case, ms):
    """(bytes, clipped mask) of the contract's decimation of the whole of file_of(case, ms)."""
    key = ("decimated", case.scene.name, case.D, case.L, int(ms))
    if key not in _CACHE:
        _CACHE[key] = spec.quantise(spec.sums(file_of(case, ms), case.taps, case.lanes, case.D), case.shift)
    return _CACHE[key]


def prepared_head(case, ms, frames):
    """(decimated bytes, clipped, prepared record) that the contracts make of the first frames * D frames of
    file_of(case, ms) - what spec.decimate and prepared_of give on that head, without filtering all of it again for every
    length: an output depends on the input within the filter's reach only, so the head's outputs are the whole file's but
    for the last few, which see the zeros behind the head, and those few are made anew from the head's end."""
    b = file_of(case, ms)
    lanes, D = case.lanes, case.D
    head = b[:frames * D * lanes]
    assert head.size == frames * D * lanes
    whole, over = _decimated_whole(case, ms)
    K = (case.L - 1) // 2 // D + 2                       # output frames whose window reaches beyond the head
    lo = max(0, frames - 2 * K - 2)                      # ... made anew with as many again in front of them
    y, clipped = whole[:frames * lanes].copy(), int(np.count_nonzero(over[:lo * lanes]))
    end, end_over = spec.quantise(spec.sums(head[lo * D * lanes:], case.taps, lanes, D), case.shift)
    if lo == 0:
        y[:], clipped = end, int(np.count_nonzero(end_over))
    else:
        keep = (frames - lo - K) * lanes                 # where the last K output frames start in `end`
        assert np.array_equal(end[keep - lanes:keep], y[keep - lanes + lo * lanes:keep + lo * lanes])   # (the seam agrees)
        y[-K * lanes:] = end[-K * lanes:]
        clipped += int(np.count_nonzero(over[lo * lanes:(frames - K) * lanes])) + int(np.count_nonzero(end_over[keep:]))
    if lanes == 1:
        return y, clipped, y
    key = ("converted", case.scene.name, case.D, case.L, int(ms))
    if key not in _CACHE:
        _CACHE[key] = prepared_of(case, whole)
    h, S = iq_spec.design(IQ_TAPS)
    M = K + IQ_TAPS                                      # pairs whose conversion sees the end of the head
    start = max(0, frames - 2 * M) & ~1                  # an even pair: the quarter-rate carrier starts over there
    want = _CACHE[key][:frames * 2].copy()
    tail = iq_spec.convert(y[2 * start:], h, S)
    if start == 0:
        want[:] = tail
    else:
        want[-2 * M:] = tail[-2 * M:]
    return y, clipped, want


def contract_acquisition(case, skip_groups=0):
    """oracle.acquire on 11 code periods of the contracts' prepared record, from output frame skip_groups on."""
    key = ("acq", case.scene.name, case.D, case.L, int(skip_groups))
    if key not in _CACHE:
        o = case.oracle_settings()
        skip = int(skip_groups) * case.lanes
        window = prepared(case, ACQ_MS)[skip:skip + 11 * o.samplesPerCode]
        assert window.size == 11 * o.samplesPerCode
        _CACHE[key] = orc.acquire(o, window)
    return _CACHE[key]
