"""The two scenes of the multi-antenna tests and the contracts' own preparation of them (tests/array_spec.py, and
tests/iq_spec.py behind it for the I/Q scene): four antennas, four satellites of 1.5 LSB in noise of 3 LSB per component
under a broadband jammer of 30 LSB per component that no single antenna acquires through.  (a) a real record at 16.368 Msps,
IF 4.092 MHz, the jammer +-2 MHz around the IF, K = 5 taps per antenna; (b) an I/Q record at 4.092 Msps, zero IF, the jammer
white over the band, K = 1.  Every satellite and the jammer reach antenna a with a steering phase of their own.
Deterministic and seeded; numpy and the oracle's C/A codes only.  Shared by tests/test_array_host.py (CPU: the contracts plus
the oracle alone) and tests/test_array_gpu.py."""
import numpy as np

import array_spec as spec
import iq_spec
from oracle import softgnss_oracle as orc

L1 = 1575.42e6
CHIP_RATE = 1023000.0
MARGIN = 1.2                # detected peaks stand at least this far above acqThreshold
ABSENT_MAX = 2.2            # the oracle's peak metric of every PRN the scene does not hold, against acqThreshold 2.5
NOISE_SIGMA = 3.0           # LSB per component and antenna
JAMMER_SIGMA = 30.0         # LSB per component
ACQ_MS = 12                 # code periods of the records the CPU tests look at
TRK_MS = 300                # code periods tracked end to end
SKIP_FRAMES = 1237          # the end-to-end skip, frames of all antennas
IQ_TAPS = 63                # Settings.iqTaps
ANTENNAS = 4
SUPPRESSION_TOL_DB = 0.5    # measured suppression against the design's prediction: tap rounding and the Toeplitz edge terms


class Scene(object):
    """lanes 1: real streams at rate fs with the carrier at f0; lanes 2: interleaved I/Q streams at the complex rate fs, the
    carrier f0 off the centre.  Per satellite a PRN, a Doppler (Hz), the instant its code starts (s), an amplitude (LSB), a
    carrier phase (rad) and a steering phase per antenna (rad); the jammer's half bandwidth (Hz; None: white) and steering."""

    def __init__(self, name, seed, lanes, fs, f0, K, prns, doppler, code_start_s, amplitude, phase, jam_half_bw):
        self.name, self.seed, self.lanes, self.fs, self.f0, self.K = name, seed, int(lanes), float(fs), float(f0), int(K)
        self.prns, self.doppler, self.code_start_s = tuple(prns), tuple(doppler), tuple(code_start_s)
        self.amplitude, self.phase, self.jam_half_bw = tuple(amplitude), tuple(phase), jam_half_bw
        rng = np.random.default_rng(seed + 7)
        self.steering = rng.uniform(-np.pi, np.pi, (len(self.prns), ANTENNAS))     # psi[i, a]
        self.steering[:, 0] = 0.0
        self.jam_steering = np.concatenate([[0.0], rng.uniform(-np.pi, np.pi, ANTENNAS - 1)])

    @property
    def frames_per_ms(self):
        return int(round(self.fs / 1000.0))

    def prepared_rate(self):
        """(samplingFreq, IF) of the prepared record: the combined one, for I/Q its real equivalent."""
        return iq_spec.real_equivalent(self.fs, self.f0) if self.lanes == 2 else (self.fs, self.f0)

    def settings(self, m, **kw):
        """The package's settings of the FILE."""
        s = m.Settings()
        s.samplingFreq, s.IF, s.iqRecord, s.iqTaps = self.fs, self.f0, self.lanes == 2, IQ_TAPS
        s.antennas = ANTENNAS
        s.numberOfChannels = len(self.prns)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def oracle_settings(self, **kw):
        fs_p, if_p = self.prepared_rate()
        return orc.OracleSettings(samplingFreq=fs_p, IF=if_p, numberOfChannels=len(self.prns), **kw)

    def amplitude_out(self, i, weights, gain):
        """The amplitude of satellite i's carrier in the combined record: amplitude x gain x |sum_a H_a(f) e^{j psi_a}| with
        H_a the frequency response of antenna a's weights (before the gain) at the satellite's carrier."""
        w = np.asarray(weights)
        c = (w.shape[1] - 1) // 2
        f = self.f0 + self.doppler[i]
        resp = (w * np.exp(-2j * np.pi * f * (np.arange(w.shape[1]) - c) / self.fs)[None, :]).sum(axis=1)
        return self.amplitude[i] * float(gain) * float(abs(np.sum(resp * np.exp(1j * self.steering[i]))))


SCENE_REAL = Scene("real_16368", 0xA88AB, 1, 16368000.0, 4092000.0, 5, (3, 11, 19, 27), (1530.0, -2260.0, 3115.0, -640.0),
                   (146.65e-6, 620.4e-6, 40.78e-6, 904.2e-6), (1.5, 1.5, 1.5, 1.5), (0.3, 1.9, -2.2, 0.8), 2.0e6)
SCENE_IQ = Scene("iq_4092", 0xA88A7, 2, 4092000.0, 0.0, 1, (3, 11, 19, 27), (-3370.0, 880.0, 2405.0, -1515.0),
                 (311.9e-6, 85.7e-6, 726.3e-6, 533.1e-6), (1.5, 1.5, 1.5, 1.5), (-1.1, 0.4, 2.6, -0.2), None)
# (the seeds were picked on the CPU so that the oracle alone, on antenna 0 and on the contracts' combined records, meets the
# conditions tests/test_array_host.py asserts, in both windows the end-to-end tests acquire in and with the weights of the
# first ACQ_MS code periods as with those of the whole file)
SCENES = {"real": SCENE_REAL, "iq": SCENE_IQ}
# The suppression of the reference antenna's power MEASURED on the contract's output bytes of the first ACQ_MS code periods
# (mean square of antenna 0 over mean square of the output / gain^2), dB, next to the design's prediction on the same
# statistics; tests/test_array_host.py holds the two within SUPPRESSION_TOL_DB of each other and these to 0.01 dB.
MEASURED_SUPPRESSION_DB = {"real": 17.2491, "iq": 17.0069}      # (the design predicts 17.2517 and 17.0091)
_CACHE = {}


def record(scene):
    """int8 bytes of the scene's file, TRK_MS + 4 code periods: frames of ANTENNAS x lanes bytes.  A shorter record is a
    prefix of it (head)."""
    key = ("file", scene.name)
    if key in _CACHE:
        return _CACHE[key]
    ms = TRK_MS + 4
    frames = ms * scene.frames_per_ms
    rng = np.random.default_rng(scene.seed)
    t = np.arange(frames, dtype=np.float64) / scene.fs
    # the jammer's complex envelope: white, or cut to +-jam_half_bw in the frequency domain and scaled back to its sigma
    jam = rng.standard_normal(frames) + 1j * rng.standard_normal(frames)
    if scene.jam_half_bw is not None:
        spectrum = np.fft.fft(jam)
        spectrum[np.abs(np.fft.fftfreq(frames, 1.0 / scene.fs)) > scene.jam_half_bw] = 0.0
        jam = np.fft.ifft(spectrum)
        jam /= np.sqrt(np.mean(np.abs(jam) ** 2) / 2.0)
    # (a real stream takes the real part of the envelope on its carrier: cos and sin rails of sigma each give sigma)
    jam *= JAMMER_SIGMA * (np.exp(2j * np.pi * scene.f0 * t) if scene.lanes == 1 else 1.0)
    sats = []
    for i, prn in enumerate(scene.prns):
        code = orc.generate_ca_code(prn - 1)
        bits = np.random.default_rng(scene.seed + 100 + prn).integers(0, 2, ms // 20 + 3) * 2 - 1
        chips = (t - scene.code_start_s[i]) * CHIP_RATE * (1.0 + scene.doppler[i] / L1)
        period = np.floor(chips / 1023.0).astype(np.int64)
        data = bits[(period + 27) // 20]         # the first edge lies behind the 11 ms that acquisition reads
        chip = code[np.floor(chips).astype(np.int64) % 1023]
        sats.append(scene.amplitude[i] * chip * data * np.exp(1j * (2.0 * np.pi * (scene.f0 + scene.doppler[i]) * t
                                                                   + scene.phase[i])))
    out = np.empty((frames, ANTENNAS, scene.lanes), dtype=np.int8)
    for a in range(ANTENNAS):
        z = jam * np.exp(1j * scene.jam_steering[a])
        for i in range(len(sats)):
            z = z + sats[i] * np.exp(1j * scene.steering[i, a])
        z = z + NOISE_SIGMA * (rng.standard_normal(frames) + 1j * rng.standard_normal(frames))
        out[:, a, 0] = np.clip(np.rint(z.real), -128, 127)
        if scene.lanes == 2:
            out[:, a, 1] = np.clip(np.rint(z.imag), -128, 127)
    b = out.reshape(-1)
    b.setflags(write=False)
    _CACHE[key] = b
    return b


def head(scene, frames, first=0):
    """Frames [first, first + frames) of the scene's file."""
    w = ANTENNAS * scene.lanes
    b = record(scene)[first * w:(first + frames) * w]
    assert b.size == frames * w
    return b


def antenna(b, scene, a):
    """The bytes of antenna a alone: a single-antenna file of the scene's kind."""
    return np.ascontiguousarray(b.reshape(-1, ANTENNAS, scene.lanes)[:, a, :]).reshape(-1)


def prepared_of(scene, stream):
    """The prepared record the contracts make of one stream: itself, or for I/Q its conversion to real IF."""
    if scene.lanes == 1:
        return stream
    h, S = iq_spec.design(IQ_TAPS)
    return iq_spec.convert(stream, h, S)


def combined(scene, frames, first=0, ref=0):
    """What the contracts make of head(scene, frames, first): dict(rho, taps, shift, gain, suppression_db, weights,
    combined (the int8 record), clipped, prepared (what every later stage reads))."""
    key = ("combined", scene.name, int(frames), int(first), int(ref))
    if key not in _CACHE:
        b = head(scene, frames, first)
        rho = spec.stats(b, scene.lanes, ANTENNAS, scene.K)
        taps, shift, gain, supp, weights = spec.design(rho, frames, scene.lanes, ref)
        y, clipped = spec.combine(b, taps, shift, scene.lanes, ANTENNAS)
        y.setflags(write=False)
        _CACHE[key] = dict(rho=rho, taps=taps, shift=shift, gain=gain, suppression_db=supp, weights=weights, combined=y,
                           clipped=clipped, prepared=prepared_of(scene, y))
    return _CACHE[key]


def measured_suppression_db(scene, frames, first=0):
    """Mean square of antenna 0 over mean square of the contract's output bytes / gain^2, dB."""
    c = combined(scene, frames, first)
    x = antenna(head(scene, frames, first), scene, 0).astype(np.float64)
    y = c["combined"].astype(np.float64)
    return float(10.0 * np.log10(np.mean(x ** 2) / (np.mean(y ** 2) / c["gain"] ** 2)))


def acquisition(scene, record8, skip=0):
    """oracle.acquire on 11 code periods of a prepared record, from sample `skip` on."""
    o = scene.oracle_settings()
    window = record8[skip:skip + 11 * o.samplesPerCode]
    assert window.size == 11 * o.samplesPerCode
    return orc.acquire(o, window)
