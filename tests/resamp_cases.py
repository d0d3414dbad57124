"""The two scenes of the resampling tests and the contract's own preparation of them (tests/resamp_spec.py): (a) a real
capture at 4.096 Msps with the IF at 1.0 MHz, brought to 40.96 Msps by 10 / 1; (b) a real capture at 16.368 Msps with the IF
at 4.092 MHz, brought to 38.192 Msps by 7 / 3.  Four satellites each, built as tests/decim_cases.py builds its scenes
(its Scene and record(): noise sigma 12, navigation bits, code Doppler).  Deterministic and seeded; numpy and the oracle's C/A
codes only.  Shared by tests/test_resamp_host.py (CPU: the contract plus the oracle alone) and tests/test_resamp_gpu.py."""
import decim_cases as dc
import resamp_spec as spec
from oracle import softgnss_oracle as orc

MARGIN = dc.MARGIN              # detected peaks stand at least this far above acqThreshold
CARR_TOL_HZ = dc.CARR_TOL_HZ    # carrFreq against the truth
PHASE_TOL = dc.PHASE_TOL        # code phase against the truth, samples of the INPUT record: times L / M at the new rate
ABSENT_MAX = dc.ABSENT_MAX      # the oracle's peak metric of every PRN the scene does not hold, against acqThreshold 2.5
ACQ_MS = 12                     # code periods of the records the CPU tests look at
TRK_MS = 200                    # code periods tracked end to end
SKIP_UNITS = 1237               # the end-to-end skip: that many groups of M input samples


class Case(object):
    """A scene and a pair L / M: what Settings.resampleUp, resampleDown and the defaults make of the file."""

    def __init__(self, scene, L, M):
        self.scene, self.L, self.M = scene, int(L), int(M)
        self.taps, self.shift, self.fs_out = spec.design(scene.fs, L, M)
        self.n_taps = self.taps.size

    def true_carrier(self, i):
        return self.scene.f0 + self.scene.doppler[i]

    def true_phase(self, i):
        """Satellite i's code phase in samples of the resampled record."""
        return self.scene.code_start_s[i] * self.fs_out

    def skip_in(self, units):
        return int(units) * self.M

    def skip_out(self, units):
        return int(units) * self.L

    def settings(self, m, **kw):
        """The package's settings of the FILE."""
        s = m.Settings()
        s.samplingFreq, s.IF = self.scene.fs, self.scene.f0
        s.resampleUp, s.resampleDown = self.L, self.M
        s.numberOfChannels = len(self.scene.prns)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def oracle_settings(self, **kw):
        return orc.OracleSettings(samplingFreq=self.fs_out, IF=self.scene.f0, numberOfChannels=len(self.scene.prns), **kw)


# (the noise seeds were picked on the CPU so that the oracle alone, on the contract's records, finds the four satellites at
# least MARGIN above the threshold and stays at or below ABSENT_MAX on all 28 PRNs that are absent, in both windows the
# end-to-end tests acquire in - at the start and behind SKIP_UNITS groups: tests/test_resamp_host.py asserts it)
SCENE_A = dc.Scene("real_4096", 0x5A3FB, 1, 4096000.0, 1000000.0, (4, 9, 17, 30), (2210.0, -1480.0, 3340.0, -590.0),
                   (212.4e-6, 731.9e-6, 55.3e-6, 468.8e-6), (7.0, 6.5, 6.0, 7.0), (0.7, -1.3, 2.1, -0.4))
SCENE_B = dc.Scene("real_16368", 0x5A3F8, 1, 16368000.0, 4092000.0, (2, 13, 21, 28), (-2870.0, 1120.0, 2655.0, -1935.0),
                   (402.6e-6, 97.1e-6, 655.0e-6, 840.3e-6), (6.0, 5.5, 5.0, 6.0), (-0.9, 0.2, 2.8, -0.6))
CASES = {
    "x10_4096": Case(SCENE_A, 10, 1),
    "x7_3_16368": Case(SCENE_B, 7, 3),
}
_CACHE = {}


def file_of(case, ms):
    return dc.record(case.scene, ms)


def prepared(case, ms):
    """(the contract's resampled record of file_of(case, ms), its clip count)."""
    key = (case.scene.name, case.L, case.M, int(ms))
    if key not in _CACHE:
        y, clipped = spec.resample(file_of(case, ms), case.taps, case.shift, case.L, case.M)
        y.setflags(write=False)
        _CACHE[key] = (y, clipped)
    return _CACHE[key]


def contract_acquisition(case, units=0):
    """oracle.acquire on 11 code periods of the contract's resampled record, from output sample units L on."""
    key = ("acq", case.scene.name, case.L, case.M, int(units))
    if key not in _CACHE:
        o = case.oracle_settings()
        skip = case.skip_out(units)
        window = prepared(case, ACQ_MS)[0][skip:skip + 11 * o.samplesPerCode]
        assert window.size == 11 * o.samplesPerCode
        _CACHE[key] = orc.acquire(o, window)
    return _CACHE[key]
