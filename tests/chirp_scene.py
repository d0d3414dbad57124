"""One scene for the swept-interference excision stage: 12 ms at the default front end (38.192 Msps, IF 9.548 MHz) of the
default satellites (synth.Scene.default's PRNs, Dopplers and code starts, each at 55 dB-Hz in Gaussian noise of 10 LSB,
tests/weak_scene.py) under a sawtooth chirp of 70 LSB that sweeps the 10 MHz around the IF every 20 us - what a "privacy"
jammer does.  Jammer over noise is 14 dB; noise, satellites and chirp together stay below the int8 rails (no sample of the
record is on one).

With the numpy contract (tests/excise_spec.py, the default segment, threshold and passes) and the oracle's acquisition
alone, tests/test_excise_host.py asserts:
  raw record      0 of the 8 satellites found (largest peak metric 1.6 against the threshold 2.5);
  excised record  8 of 8, on the code phases and Doppler bins of the search without the chirp (smallest metric 5.7; 10.0 ..
                  14.2 without the chirp), with 13.4 % of the time-frequency cells cut.
The default Dopplers lie near ties of the 500 Hz grid (1250 Hz is exactly between two bins), so which bin the noise picks
is a property of the seed: it is fixed here where the clean and the excised search agree.  Everything is computed once per
process and never changed."""
import numpy as np

import excise_spec as spec
import weak_scene
from oracle import softgnss_oracle as orc

MS = 12.0
PRNS = (1, 3, 7, 11, 14, 19, 22, 31)                       # synth.Scene.default()
DOPPLERS = (1250, -3100, 4800, -650, 2900, -4400, 350, -1900)
CODE_STARTS = (12345, 30001, 5, 20000, 777, 38000, 15000, 9000)
CN0 = 55.0
SIGMA = 10.0
SEED = 3
CHIRP_AMPLITUDE = 70.0
CHIRP_SPAN_HZ = 10e6
CHIRP_PERIOD_S = 20e-6
PRN_INDICES = [p - 1 for p in PRNS]

_cache = {}


def settings():
    return orc.OracleSettings()


def clean():
    if "clean" not in _cache:
        sats = tuple((p - 1, CN0, float(d), s0) for p, d, s0 in zip(PRNS, DOPPLERS, CODE_STARTS))
        x = weak_scene.generate(MS, sats=sats, seed=SEED, sigma=SIGMA, nav_bits=False)
        x.setflags(write=False)
        _cache["clean"] = x
    return _cache["clean"]


def chirp(n, fs=weak_scene.FS, if_=weak_scene.IF):
    """The sawtooth: from IF - span / 2 to IF + span / 2 over one period, then back at once."""
    period = CHIRP_PERIOD_S * fs
    t = np.arange(n, dtype=np.float64) % period
    f0, f1 = (if_ - CHIRP_SPAN_HZ / 2.0) / fs, (if_ + CHIRP_SPAN_HZ / 2.0) / fs
    return CHIRP_AMPLITUDE * np.cos(2.0 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / period))


def record():
    """The int8 record with the chirp on it."""
    if "record" not in _cache:
        c = clean()
        x = np.clip(c + np.rint(chirp(c.size)), -127, 127).astype(np.int8)
        x.setflags(write=False)
        _cache["record"] = x
    return _cache["record"]


def excised(N=256, threshold=8.0, passes=3):
    """(y, info) of the contract on the record."""
    key = ("excised", N, threshold, passes)
    if key not in _cache:
        y, info = spec.excise(record(), N, threshold, passes)
        y.setflags(write=False)
        _cache[key] = (y, info)
    return _cache[key]


def search(which):
    """The oracle's acquisition of the scene's PRNs on 'clean', 'raw' or 'excised'."""
    key = ("search", which)
    if key not in _cache:
        x = {"clean": clean, "raw": record, "excised": lambda: excised()[0]}[which]()
        s = settings()
        _cache[key] = orc.acquire(s, x[:11 * s.samplesPerCode], prn_indices=PRN_INDICES)
    return _cache[key]
