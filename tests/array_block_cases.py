"""The moving-jammer scene of the block-adaptive combiner's tests and the contracts' own preparation of it (tests/
array_block_spec.py on tests/array_spec.py, tests/iq_spec.py behind them): tests/array_cases.py's I/Q scene - four antennas,
four satellites of 1.5 LSB under a white jammer of 30 LSB per component, 4.092 Msps, K = 1 - with ONE change: the jammer's
steering phase on antenna a runs on as psi_a + 2 pi RATE_HZ a t, a jammer that drives past.  Over the RECORD_MS the tests
read, antenna 3 moves 1.9 rad: one null for the whole record points nowhere, a null per millisecond follows.  Deterministic
and seeded; numpy and the oracle's C/A codes only.  Shared by tests/test_array_block_host.py (CPU: the contracts plus the
oracle alone) and tests/test_array_block_gpu.py."""
import numpy as np

import array_block_spec as bspec
import array_cases as cases
import array_spec as spec
from oracle import softgnss_oracle as orc

RATE_HZ = 0.8               # the jammer's steering phase on antenna a turns at a x this
SEED = 0xA88A7              # array_cases.SCENE_IQ's
# (seed and rate are the first pair tried: with them the oracle alone, on the contracts' records, meets every condition
# tests/test_array_block_host.py asserts in all three windows - checked on the CPU as array_cases' seeds were; at 1.5 and
# 3 Hz the adaptive null passes over one satellite's own direction for a while and that satellite fades, which is inherent
# in power inversion and what the scene stays clear of)
RECORD_MS = 124             # code periods of the file
BLOCK_MS = 1.0              # Settings.arrayBlockMs: blocks of 4096 frames at 4092 frames per ms
WINDOW = 3                  # Settings.arrayWindowBlocks
TRK_MS = 100                # code periods tracked end to end
WINDOWS_MS = (0, 55, 110)   # where acquisition looks: the start, the middle and the end of the file
MARGIN, ABSENT_MAX, ANTENNAS, SKIP_FRAMES = cases.MARGIN, cases.ABSENT_MAX, cases.ANTENNAS, cases.SKIP_FRAMES
RMS_TOL = 0.02              # output rms per block against arrayTargetRms
_CACHE = {}


class MovingScene(cases.Scene):
    """array_cases.SCENE_IQ with a jammer whose steering phase runs on: jam_steering[a] is a series over the frames of
    array_cases.record(), which multiplies it in frame by frame."""

    def __init__(self, name, seed, rate_hz):
        iq = cases.SCENE_IQ
        cases.Scene.__init__(self, name, seed, iq.lanes, iq.fs, iq.f0, iq.K, iq.prns, iq.doppler, iq.code_start_s,
                             iq.amplitude, iq.phase, iq.jam_half_bw)
        self.rate_hz = float(rate_hz)
        t = np.arange((cases.TRK_MS + 4) * self.frames_per_ms, dtype=np.float64) / self.fs
        self.jam_steering = self.jam_steering[:, None] + 2.0 * np.pi * self.rate_hz * np.arange(ANTENNAS)[:, None] * t[None, :]


SCENE = MovingScene("iq_4092_moving", SEED, RATE_HZ)
FRAMES = RECORD_MS * SCENE.frames_per_ms
BLOCK_FRAMES = max(1, int(round(BLOCK_MS * SCENE.fs / 1000.0 / bspec.BLOCK_UNIT))) * bspec.BLOCK_UNIT


def record(scene=SCENE):
    """int8 bytes of the file: the first RECORD_MS code periods of array_cases.record(scene)."""
    return cases.head(scene, RECORD_MS * scene.frames_per_ms)


def combined_whole(scene, frames, first=0):
    """What today's path makes of frames [first, first + frames) of the file: array_cases.combined, one set of weights."""
    return cases.combined(scene, frames, first)


def combined_blocks(scene, frames, first=0, B=None, W=WINDOW, ref=0):
    """What the block contracts make of frames [first, first + frames) of the file, blocks counted from `first`: dict(rho
    (per block), taps, shift, gain, suppression_db, weights, status (all per block), combined (the int8 record), clipped,
    prepared (what every later stage reads))."""
    B = BLOCK_FRAMES if B is None else B
    key = ("blocks", scene.name, int(frames), int(first), int(B), int(W), int(ref))
    if key not in _CACHE:
        b = cases.head(scene, frames, first)
        rho = bspec.block_stats(b, scene.lanes, ANTENNAS, scene.K, B)
        taps, shift, gain, supp, weights, status = bspec.design_blocks(rho, frames, B, W, scene.lanes, ref)
        y, clipped = bspec.combine_blocks(b, taps, B, shift, scene.lanes, ANTENNAS)
        y.setflags(write=False)
        _CACHE[key] = dict(rho=rho, taps=taps, shift=shift, gain=gain, suppression_db=supp, weights=weights, status=status,
                           combined=y, clipped=clipped, prepared=cases.prepared_of(scene, y))
    return _CACHE[key]


def acquisition(scene, prepared, ms):
    """oracle.acquire on the 11 code periods of a prepared record that start `ms` code periods of the file in."""
    return cases.acquisition(scene, prepared, ms * scene.frames_per_ms * scene.lanes)


def tracked(scene, prepared, ms=TRK_MS):
    """(the oracle's acquisition at the start of a prepared record, its channel table, its stacked series of `ms` code
    periods)."""
    o = scene.oracle_settings(msToProcess=float(ms))
    ref = orc.acquire(o, prepared[:11 * o.samplesPerCode])
    chans = orc.pre_run(o, ref)
    return ref, chans, orc.stack_series(orc.track(o, chans, prepared))
