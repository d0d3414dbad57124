"""Sampling rates whose samplesPerCode has a prime factor above 31 (csrc/sgx_acq.hip, acquire_passes on a padded
length): the scenes and searches tests/test_any_rate_gpu.py asserts on the GPU, the padded search in numpy (the design's
premise: the reference's circular correlation inside a longer one), and what tests/test_any_rate_host.py needs to show that
every one of those searches is well conditioned in numpy alone.  Everything is numpy from fixed seeds."""
import numpy as np

import coherent_acq_spec as spec
import dense_scene
from conftest import pkg
from oracle import softgnss_oracle as orc

# (samplingFreq, IF): 53 000 = 2^3 5^3 53, 37 000 = 2^3 5^3 37, 5 714 = 2 2857, 4 099 is prime
RATES = [(53000000.0, 14580000.0), (37000000.0, 9250000.0), (5714000.0, 1430000.0), (4099000.0, 1025000.0)]
RATE_IDS = ["53.0", "37.0", "5.714", "4.099"]
SMOOTH_IN_USE = [38192, 16368, 5456, 4092, 61380, 60000, 26000, 20460, 12276]   # samplesPerCode of the suite's other rates
PRNS = list(range(1, 7))      # acqSatelliteList of every search here
GAP = 1e-6                    # smallest relative distance of an asserted arg-max from its runner-up
THRESHOLD_ROOM = 0.01         # no peakMetric within 1 % of acqThreshold


def smooth(m):
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31):
        while m % p == 0:
            m //= p
    return m == 1


def oracle_settings(fs, IF, **kw):
    return orc.OracleSettings(samplingFreq=fs, IF=IF, acqSatelliteList=PRNS, numberOfChannels=2, msToProcess=50.0, **kw)


def settings(fs, IF, **kw):
    s = pkg().Settings()
    s.samplingFreq, s.IF = fs, IF
    s.acqSatelliteList = PRNS
    s.numberOfChannels = 2
    s.msToProcess = 50.0
    for k, v in kw.items():
        setattr(s, k, v)
    return s


_RECORDS = {}


def record(fs, IF):
    """The scene of test_other_front_ends_against_oracle at this rate: PRNs 2 and 5, 50 ms + the acquisition window."""
    if fs not in _RECORDS:
        synth = pkg("synth")
        n = int(round(fs / 1000))
        sc = synth.Scene.make(0xFE000 + n, fs, IF, [2, 5], [1750.0, -3300.0], [n // 3, n - 5], [9, 8])
        _RECORDS[fs] = synth.generate(sc, synth.record_length(n, 50))
    return _RECORDS[fs]


def padded_peaks(s, x, length, p, n_blocks=2, noncoh=False):
    """One PRN's search grid res[bin, sample] of acquisition.py:99-133 with every transform of length `length` >= 2 N - 1:
    the mixed block in the first N entries of a zero row, the code row with its wrap-around copy code[1 .. N - 1] at the
    row's end, the first N outputs of ifft(fft(x') conj(fft(c'))) kept."""
    n = s.samplesPerCode
    assert length >= 2 * n - 1
    ts = 1.0 / s.samplingFreq
    phase_points = np.arange(n) * 2 * np.pi * ts
    code = orc.make_ca_table(s)[p]
    crow = np.zeros(length)
    crow[:n] = code
    crow[length - n + 1:] = code[1:]
    code_fd = np.fft.fft(crow).conj()
    bins = orc.freq_bins(s)
    res = np.zeros((len(bins), n))
    for k, f in enumerate(bins):
        pw = []
        for b in range(n_blocks):
            blk = x[b * n:(b + 1) * n]
            row = np.zeros(length, dtype=np.complex128)
            row[:n] = np.sin(f * phase_points) * blk + 1j * (np.cos(f * phase_points) * blk)
            pw.append(abs(np.fft.ifft(np.fft.fft(row) * code_fd)[:n]) ** 2)
        if noncoh:
            acc = pw[0]
            for q in pw[1:]:
                acc = acc + q
            res[k] = acc
        else:
            best = 0
            for b in range(1, n_blocks):
                if not (pw[best].max() > pw[b].max()):
                    best = b
            res[k] = pw[best]
    return res


def padded_acquire(s, x, length, prn_indices, n_blocks=2, noncoh=False):
    """freqBin, codePhase of the peak and peakMetric (acquisition.py:135-164) from padded_peaks, per PRN index."""
    n = s.samplesPerCode
    spc = int(round(s.samplingFreq / s.codeFreqBasis))
    out = {}
    for p in prn_indices:
        res = padded_peaks(s, np.asarray(x, dtype=np.float64), length, p, n_blocks, noncoh)
        fbi = int(res.max(1).argmax())
        c = int(res.max(0).argmax())
        second = res[fbi, orc.exclusion_index(c, n, spc)].max()
        out[p] = (fbi, c, res.max(0).max() / second)
    return out


# ---- the 1-ms searches of the GPU file, each as (name, rate index, signal, n_blocks, noncoh) ----
def scaled(x):
    return x.astype(np.float64) * 0.37 + 0.123


OFFSET = 12345   # not a multiple of 16


def search_cases():
    out = []
    for i, (fs, IF) in enumerate(RATES):
        n = int(round(fs / 1000))
        out.append(("scene_" + RATE_IDS[i], i, lambda fs=fs, IF=IF, n=n: record(fs, IF)[:11 * n], 2, False))
    n = 5714
    out.append(("noncoh10_5.714", 2, lambda: record(*RATES[2])[:20 * n], 10, True))
    n = 4099
    out.append(("f64_4.099", 3, lambda: scaled(record(*RATES[3])[:11 * n]), 2, False))
    n = 37000
    out.append(("offset_37.0", 1, lambda: record(*RATES[1])[OFFSET:OFFSET + 11 * n], 2, False))
    return out


def conditioned(s, x, n_blocks, noncoh, prns=None):
    """spec.acquire (the 1-ms grid: oracle.acquire's search) with what decides every arg-max.  Returns (outputs, smallest
    relative gap over the bin, sample and fine arg-maxes of every searched PRN, closest |peakMetric / threshold - 1|).
    prns: the searched PRNs (default: PRNS)."""
    prns = PRNS if prns is None else prns
    w = spec.acquire(s, x, 1, n_blocks, noncoh, 500.0, prn_indices=[p - 1 for p in prns], details=True)
    gaps, room = [], []
    for p in (q - 1 for q in prns):
        d = w["details"][p]
        gaps += [spec.rel_gap(d["bins"]), spec.rel_gap(d["samples"])]
        if d["fine"] is not None:
            gaps.append(spec.rel_gap(d["fine"]))
        room.append(abs(w["peakMetric"][p] / s.acqThreshold - 1.0))
    return w, min(gaps), min(room)


# ---- code-phase edges on a padded length: N = 5 714, 6 samples per chip ----
EDGE_RATE = RATES[2]
EDGE_N, EDGE_SPC = 5714, 6
EDGE_PHASES = [0, 1, EDGE_SPC - 1, EDGE_SPC, EDGE_SPC + 1, EDGE_N - 1 - EDGE_SPC, EDGE_N - EDGE_SPC, EDGE_N - 1]
EDGE_CODE_START = {c: (c - 1) % EDGE_N for c in EDGE_PHASES}   # the peak lies one sample behind the code's start


def edge_settings(oracle=True):
    fs, IF = EDGE_RATE
    if oracle:
        return orc.OracleSettings(samplingFreq=fs, IF=IF, acqSatelliteList=[1])
    s = pkg().Settings()
    s.samplingFreq, s.IF, s.acqSatelliteList = fs, IF, [1]
    return s


def edge_record(c):
    fs, IF = EDGE_RATE
    synth = pkg("synth")
    sc = synth.Scene.make(0xED6E0000 + c, fs, IF, [1], [1500], [EDGE_CODE_START[c]], [10])
    return synth.generate(sc, 11 * EDGE_N)


# ---- coherent search, direct path, on a padded length ----
COHERENT_CASES = [
    dense_scene.Case("fs5714_2x2_ref", 2, 2, fs=5714000.0, if_=1430000.0, seed=21, path="direct", prn_chunk=17),
    dense_scene.Case("fs5714_2x2_noncoh", 2, 2, noncoh=True, fs=5714000.0, if_=1430000.0, seed=22, path="direct",
                     prn_chunk=17),
]
COHERENT_BY_NAME = {c.name: c for c in COHERENT_CASES}
