"""Scenes shared by the coherent-tracking tests (plain numpy): one or more C/A satellites with random data bits on a
known bit edge, Gaussian noise, int8.  tests/test_coh_track_cases.py shows on the CPU that they are well-conditioned;
tests/test_coh_track_gpu.py runs the kernel on them.

Sample n holds  sum_sat A(n) d(n) c(n) sin(2 pi (IF + doppler) n / fs + phase) + noise:  the code starts at sample
`start` and runs at codeFreqBasis (1 + doppler / 1575.42e6); bit b covers the code periods edge + 20 b ... edge + 20 b + 19
(the periods in front of `edge` carry a bit of their own).  C/N0 = A^2 fs / (4 sigma^2).
"""
import numpy as np

from oracle import softgnss_oracle as orc

FS_LOW, IF_LOW = 4.092e6, 1.0e6
SIGMA = 20.0
L1 = 1575.42e6
F_SEEDS = (1, 2, 3, 4, 5, 6)          # scene F: the seeds of the CPU test; the GPU test runs the first two
CHUNK = 1 << 20


def amplitude(cno_dbhz, fs, sigma=SIGMA):
    return float(np.sqrt(4.0 * sigma * sigma * 10.0 ** (cno_dbhz / 10.0) / fs))


def settings(fs=FS_LOW, IF=IF_LOW, **kw):
    return orc.OracleSettings(samplingFreq=fs, IF=IF, **kw)


def make_record(seed, fs, IF, n_samples, sats, sigma=SIGMA):
    """sats: dicts(prn, doppler, start, edge, phase, cno: dB-Hz or (dB-Hz of the first `fade_at` code periods, dB-Hz
    behind them), fade_at).  -> (int8[n_samples], bits per satellite: +-1 per code period as int8)."""
    rng = np.random.default_rng(seed)
    n_periods = int(n_samples * 1.023e6 / fs / 1023) + 3
    plans = []
    for sat in sats:
        data = rng.integers(0, 2, n_periods // 20 + 3) * 2 - 1
        per = np.arange(n_periods)
        bits = data[(per - sat["edge"]) // 20 + 1].astype(np.int8)
        cno = sat["cno"]
        amp = np.full(n_periods, amplitude(cno if np.isscalar(cno) else cno[1], fs, sigma))
        if not np.isscalar(cno):
            amp[:sat["fade_at"]] = amplitude(cno[0], fs, sigma)
        plans.append((orc.generate_ca_code(sat["prn"] - 1), bits, amp))
    out = np.empty(n_samples, dtype=np.int8)
    for lo in range(0, n_samples, CHUNK):
        n = np.arange(lo, min(lo + CHUNK, n_samples), dtype=np.float64)
        x = rng.normal(0.0, sigma, n.size)
        for sat, (code, bits, amp) in zip(sats, plans):
            chips = (n - sat["start"]) * (1.023e6 * (1.0 + sat["doppler"] / L1) / fs)
            whole = np.floor(chips)
            per = np.floor(whole / 1023.0)
            idx = (whole - 1023.0 * per).astype(np.int64)
            per = np.clip(per.astype(np.int64), 0, bits.size - 1)
            live = chips >= 0
            turns = (IF + sat["doppler"]) / fs * n
            x += live * amp[per] * bits[per] * code[idx] * np.sin(2.0 * np.pi * (turns - np.floor(turns)) + sat["phase"])
        out[lo:lo + n.size] = np.clip(np.rint(x), -127, 127).astype(np.int8)
    return out, [p[1] for p in plans]


# ---- scene F, the fade: 42 dB-Hz for one second, 26 dB-Hz afterwards -----------------------------------------------------------
F = dict(prn=5, doppler=1234.0, start=123, edge=7, phase=0.7, cno=(42.0, 26.0), fade_at=1000)
F_MS = 4000


def scene_f(seed):
    """-> (settings, record, bits per code period, the channel handed to tracking (prn, acquiredFreq, codePhase))."""
    s = settings()
    n = int(F_MS * 4092 + 3 * 4092)
    rec, bits = make_record(seed, FS_LOW, IF_LOW, n, [F])
    return s, rec, bits[0], (F["prn"], IF_LOW + F["doppler"] + 3.0, float(F["start"]))


def wrong_bits(i_p, bits, edge, first_ms):
    """Share of wrong bit decisions behind block first_ms: the sign of each 20 ms sum of I_P on the true edges against the
    bit sent (block k of a channel that starts on the code's start is code period k), up to one sign for the whole run."""
    k = first_ms + (edge - first_ms) % 20
    n = (len(i_p) - k) // 20
    got = np.sign(i_p[k:k + 20 * n].reshape(n, 20).sum(axis=1))
    sent = bits[k:k + 20 * n:20]
    bad = int(np.sum(got != sent))
    return min(bad, n - bad) / float(n)


# ---- three satellites at 45 dB-Hz with bit edges 0, 7 and 19 (the group logic and the bit synchronisation) ----------------
TRIO = (dict(prn=3, doppler=-2210.0, start=57, edge=0, phase=0.3, cno=45.0),
        dict(prn=11, doppler=640.0, start=1999, edge=7, phase=2.1, cno=45.0),
        dict(prn=22, doppler=3105.0, start=3333, edge=19, phase=4.0, cno=45.0))
TRIO_SEED = 12        # (300 ms hold 15 bits: seed 11 draws too few sign changes for the edge-19 satellite, margin 1.04)


def scene_trio(ms, fs=FS_LOW, IF=IF_LOW, seed=TRIO_SEED):
    """-> (settings, record, channels [(prn, acquiredFreq, codePhase)] + one channel that is off, true edges)."""
    s = settings(fs, IF)
    spc = s.samplesPerCode
    scale = spc / 4092.0
    sats = [dict(t, start=int(t["start"] * scale)) for t in TRIO]
    rec, _ = make_record(seed, fs, IF, int((ms + 3) * spc), sats)
    chans = [(t["prn"], IF + t["doppler"] + 2.0, float(t["start"])) for t in sats] + [(0, 0.0, 0.0)]
    return s, rec, chans, [t["edge"] for t in sats] + [0]


# Every run of tests/test_coh_track_gpu.py on this scene in which the kernel FINDS the edges and the test compares them:
# (pull-in P, skipNumberOfBytes of zeros in front of the record), ms = 400, T = 20, seed TRIO_SEED.
# tests/test_coh_track_cases.py shows a margin of at least 1.05 on each.  (P = 220 is not among them: 1.03 on the edge-19 channel.)
SYNC_MS = 400
SYNC_SCENES = ((300, 0), (307, 0), (308, 0), (260, 1000))


def scene_sync(skip):
    """The trio scene of SYNC_MS ms behind `skip` zero bytes -> (settings with that skipNumberOfBytes, record, channels, edges)."""
    s0, rec, chans, edges = scene_trio(SYNC_MS)
    s = settings(s0.samplingFreq, s0.IF, skipNumberOfBytes=skip)
    return s, (np.r_[np.zeros(skip, dtype=np.int8), rec] if skip else rec), chans, edges


def edge_margin(energy):
    """E_max / E_second of one channel's 20 bit-synchronisation energies."""
    e = np.sort(np.asarray(energy, dtype=np.float64))
    return e[-1] / e[-2]
