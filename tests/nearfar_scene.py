"""The near-far scene of the strong-signal cancellation, shared by tests/test_cancel_host.py,
tests/test_cancel_gpu.py and tests/cancel_cases.py: two strong satellites (PRN 1 and 3, amplitudes 48 and 44) beside two weak
ones (PRN 7 and 11, amplitude 3) at 16.368 Msps.  54 ms are generated; the search window is [2 n, 13 n) with
n = samplesPerCode, and the strong channels are tracked for 40 ms from the code phases it finds, taken from file offset 0
(a code period is n samples, so the phase holds there): every sample of the window lies inside their blocks.  Test
infrastructure only."""
import functools

import numpy as np

import cancel_spec as spec
import replay_spec
from conftest import pkg
from oracle import softgnss_oracle as orc

FS, IF = 16.368e6, 4.092e6
PRNS, DOPPLERS = [1, 3, 7, 11], [1000, -2000, 2000, -1000]
CODE_STARTS, AMPS = [1234, 9000, 4000, 15000], [48, 44, 3, 3]
STRONG, WEAK, ABSENT = (1, 3), (7, 11), (14, 19)
SEARCHED = STRONG + WEAK + ABSENT
MS_GENERATED, MS_TRACKED = 54, 40


def scene():
    return pkg("synth").Scene.make(0xBEEF, fs=FS, IF=IF, prns=PRNS, dopplers=DOPPLERS, code_starts=CODE_STARTS, amps=AMPS)


def settings(**kw):
    return orc.OracleSettings(samplingFreq=FS, IF=IF, numberOfChannels=2, msToProcess=float(MS_TRACKED), **kw)


@functools.lru_cache(maxsize=None)
def record():
    rec = pkg("synth").generate(scene(), MS_GENERATED * settings().samplesPerCode)
    rec.setflags(write=False)
    return rec


def search(s, rec):
    """The oracle's search of [2 n, 13 n) for the six PRNs of the scene's claims: {prn: (peakMetric, codePhase, carrFreq)}."""
    n = s.samplesPerCode
    acq = orc.acquire(s, np.asarray(rec[2 * n:13 * n]), prn_indices=[p - 1 for p in SEARCHED])
    return {p: (float(acq["peakMetric"][p - 1]), float(acq["codePhase"][p - 1]), float(acq["carrFreq"][p - 1]))
            for p in SEARCHED}


def detected(found, s):
    return sorted(p for p, (metric, _, _) in found.items() if metric > s.acqThreshold)


@functools.lru_cache(maxsize=None)
def oracle_run():
    """(settings, record, raw search, chans of PRN 1 and 3, their series [2][13][40]) with the oracle's search and tracking."""
    s, rec = settings(), record()
    found = search(s, rec)
    chans = [(p, found[p][2], found[p][1]) for p in STRONG]
    ch = dict(PRN=np.array([c[0] for c in chans]), acquiredFreq=np.array([c[1] for c in chans]),
              codePhase=np.array([c[2] for c in chans]), status=['T'] * len(chans))
    series = orc.stack_series(orc.track(s, ch, rec, ms=MS_TRACKED))
    series.setflags(write=False)
    return s, rec, found, chans, series


@functools.lru_cache(maxsize=None)
def oracle_cancelled(smooth=1):
    """(amp, y, v, clipped, covered) of the contract on the oracle's run."""
    s, rec, _, chans, series = oracle_run()
    amp = spec.design(series, spec.states(s, rec.size, 0, chans, series, None), None, smooth)
    return (amp,) + spec.cancel(s, rec, 0, chans, series, None, amp)


# The scene behind a record stage (the resident path of postProcessing): the file is the record with a DC offset, which the
# conditioning stage - byte-exact against tests/cond_spec.py - removes; the prepared record is what acquisition, tracking and
# the cancellation then read, positions being samples of it.  postProcessing() prepares the bytes it needs and no more:
# msToProcess blocks of up to n + 2 samples and two code periods.
DC_OFFSET = 5
COND = dict(condBlockUs=100.0, condAgcBlocks=32.0, condBlankFactor=4.0, condGuardFrames=8, condTargetRms=12.0)   # the defaults


@functools.lru_cache(maxsize=None)
def offset_file():
    """The record as a file whose front end adds DC_OFFSET LSB (int8, saturating)."""
    rec = np.clip(record().astype(np.int16) + DC_OFFSET, -128, 127).astype(np.int8)
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def prepared_record():
    """What Settings.conditionRecord makes of the bytes of offset_file() that postProcessing() reads, with the settings COND,
    by the stage's numpy contract."""
    import cond_spec
    n = settings().samplesPerCode
    raw = offset_file()[:MS_TRACKED * (n + 2) + 2 * n]
    block = min(16384, max(256, 16 * int(np.rint(COND["condBlockUs"] * 1e-6 * FS / 16.0))))
    blank_q4 = int(np.rint(16.0 * COND["condBlankFactor"] ** 2))
    stats = cond_spec.block_stats(raw, np.int8, 1, block, blank_q4)
    plan = cond_spec.plan(stats, 1, blank_q4, COND["condTargetRms"], COND["condAgcBlocks"])
    y = cond_spec.condition(raw, np.int8, 1, block, plan, COND["condGuardFrames"])[0]
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def oracle_run_prepared():
    """(raw search, chans, series, cleaned search) of the oracle on prepared_record(): the search, the strong channels
    tracked for 40 ms, cancelled by the contract (one amplitude pair per block), and the search of the cleaned record."""
    s, rec = settings(), prepared_record()
    found = search(s, rec)
    chans = [(p, found[p][2], found[p][1]) for p in STRONG]
    ch = dict(PRN=np.array([c[0] for c in chans]), acquiredFreq=np.array([c[1] for c in chans]),
              codePhase=np.array([c[2] for c in chans]), status=['T'] * len(chans))
    series = orc.stack_series(orc.track(s, ch, rec, ms=MS_TRACKED))
    amp = spec.design(series, spec.states(s, rec.size, 0, chans, series, None))
    y = spec.cancel(s, rec, 0, chans, series, None, amp)[0]
    return found, chans, series, search(s, y)


def prompt_power_db(s, rec, chans, series):
    """Per channel, 10 log10 of the mean prompt power I_P^2 + Q_P^2 of the channel replayed on `rec`."""
    out = []
    for c, (prn, f, cp) in enumerate(chans):
        i, q, _ = replay_spec.replay(s, rec, "int8", prn, f, cp, series[c, 0], series[c, 1], series[c, 2], series.shape[2],
                                     (0.0,))
        out.append(10.0 * np.log10(np.mean(i[0] ** 2 + q[0] ** 2)))
    return np.array(out)
