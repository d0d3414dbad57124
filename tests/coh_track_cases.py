"""Scenes shared by the coherent-tracking tests (plain numpy): one or more C/A satellites with random data bits on a
known bit edge, Gaussian noise, int8.  tests/test_coh_track_cases.py shows on the CPU that they are well-conditioned;
tests/test_coh_track_gpu.py runs the kernel on them, tests/test_coh_track_limits_gpu.py on the cases at the end of this file.

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


# ---- the limits: tests/test_coh_track_limits_gpu.py runs the kernel on what follows, tests/test_coh_track_cases.py shows on
# the CPU, with the contract alone, that a slip in each case would lie outside the GPU test's bar --------------------------

# 1. RATES.  scene_trio(110, fs, IF), ms = 110, T = 20, P = 40, H = 100, the trio's own edges: a coherent phase at rates that
# are neither 4.092 nor 38.192 Msps.  (fs, IF, units of 4096 samples the launch holds, the sample-by-sample map?):
#   5.456 Msps   5.33 samples per chip - no whole number of them (full_scale.LOW_RATE)
#   15.345 Msps  15 per chip: the last whole rate on the sample-by-sample map, four units
#   16.368 Msps  16 per chip: the one-switch map, where E, P and L switch 8 samples apart - its sample-by-sample route
#   61.38 Msps   60 per chip: 16 units, the most the kernel holds
RATE_SCENES = ((5.456e6, 1.364e6, 2, True), (15.345e6, 3.9e6, 4, True), (16.368e6, 4.1304e6, 5, False), (61.38e6, 15.3e6, 16, False))
RATE_RUN = dict(ms=110, T=20, P=40, H=100)


def trk_units(n_code):
    """csrc/sgx_trk.hip, sgx_trk_units: the units of 256 groups of 16 samples that hold the longest block, worst alignment."""
    return -(-((n_code + 94) // 16) // 256)


def trk_by_sample(fs):
    """csrc/sgx_trk.hip, sgx_trk_multi: under ~15.4 samples per chip a group of 16 can hold several switches of a ramp."""
    return 15.0 * 1.001 * 1.023e6 / fs >= 1.0


# 2. A RECORD AT AN OFFSET.  The record a call is given starts at byte `off` of the file and the channels keep their file
# positions.  A channel that starts in front of `off` is moved behind it by whole code periods (4092 samples: the code phase
# holds), and its bit edge with it - block k of the moved channel is code period k + periods of the satellite.
OFFSETS = dict(window=3 * 4096, odd=3 * 4096 + 5, large=2 ** 33 + 4096, classes=8192)
OFFSET_RUN = dict(ms=110, T=10, P=40, H=100)
OFFSET_SYNC = dict(ms=SYNC_MS, T=20, P=300, H=100)        # 2(e), TrackingResult.track: the edges are found


def moved_behind(chans, edges, off, spc=4092):
    """-> (channels, edges) with every active channel in front of file byte `off` moved behind it by whole code periods."""
    out_c, out_e = [], []
    for (prn, f, cp), e in zip(chans, edges):
        k = max(0, -(-(off - int(cp)) // spc)) if prn else 0
        out_c.append((prn, f, cp + spc * k))
        out_e.append((e - k) % 20 if prn else e)
    return out_c, out_e


# 4. MANY CHANNELS.  300 rows: 294 active ones with pairwise different carriers and edges, six that are off - at the table's
# start, around the 64 rows up to which the call's int arrays fill one 256-byte slot, and further in.  ms = 60, T = 4, H = 7.
MANY = 300
MANY_OFF = (0, 63, 64, 65, 128, 298)
MANY_RUN = dict(ms=60, T=4, P=40, H=7)


def many_channels(chans, edges, n=MANY):
    """-> (n channels, n edges): row i is satellite i % 3, (i // 3) / 4 - 10 Hz beside it, its edge moved on by i."""
    rows = [(0, 0.0, 0.0) if i in MANY_OFF else (chans[i % 3][0], chans[i % 3][1] + (i // 3) * 0.25 - 10.0, chans[i % 3][2])
            for i in range(n)]
    return rows, [(edges[i % 3] + i) % 20 for i in range(n)]


# 5. FULL SCALE.  tests/full_scale.py's records of 104 ms at its low rate and at the default front end: one whose every byte
# is -128 or 127, one noiseless at amplitude 127.  One channel, 2 Hz beside the carrier; ms = 100, T = 20, edge 3.
FULL_SCALE_RATES = ((5456000.0, 1364000.0), (38.192e6, 9.548e6))
FULL_SCALE_RUN = dict(ms=100, T=20, P=40, H=100)
FULL_SCALE_EDGE = 3


def full_scale_case(m, fs, IF, kind):
    """kind 'clipped' | 'clean' -> (oracle settings, int8 record, [channel])."""
    import full_scale as fsc
    ps = m.Settings()
    ps.samplingFreq, ps.IF = fs, IF
    rec = fsc.clipped_record(m, ps, "int8", 104) if kind == "clipped" else fsc.clean_record(m, ps, 127, 104).astype(np.int8)
    prn, f, start = fsc.clean_channel(ps)
    return settings(fs, IF), rec, [(prn, f + 2.0, float(start))]


# 6. T = 1 through the entry point: the 400 ms trio, P = 300, the edges found; k0 = -1 and the reference's series throughout.
# (P = 220 would not do: 1.03 on the edge-19 channel, as above.)
T1_RUN = dict(ms=300, T=1, P=300, H=100)

# 7. A CHANNEL THAT ENDS WHILE ITS EDGE IS SOUGHT (T = 20, P = 220, ms = 300, every edge -1): zeros from block 100 of channel 0
# on, and a record cut 100 samples into its block 150.  The edge stays -1, k0 -1, the energies are those of the whole
# 20-block sums so far.
ENDS_RUN = dict(ms=300, T=20, P=220, H=100)


def ends_early(rec, chans, how):
    at = int(chans[0][2])
    if how == "silence":
        out = rec.copy()
        out[at + 100 * 4092:] = 0
        return out
    return rec[:at + 150 * 4092 + 100]


# 8. A BLOCK BEYOND THE UNITS (tests/test_gpu_parity.py's range test): synth.Scene.default() of 80 periods at 38.192 Msps,
# two channels off any signal; ten units of 4096 samples.  dllNoiseBandwidth 2000 still fits, 6000 does not.
RANGE_CHANNELS = [(7, 9.548e6, 1234.0), (1, 9.5478e6, 12345.0)]
RANGE_RUN = dict(ms=60, T=4, P=40, H=100)
RANGE_ROOM = 10 * 4096 - 15

# 9. OTHER LOOPS.  ms = 150, T = 10: a quarter-chip spacing, and other 1 ms loops; both with coherent loops of 8 and 0.5 Hz.
LOOPS_RUN = dict(ms=150, T=10, P=40, H=100)
LOOPS_COH = dict(cohPllNoiseBandwidth=8.0, cohDllNoiseBandwidth=0.5)
LOOPS = (dict(dllCorrelatorSpacing=0.25),
         dict(pllDampingRatio=0.9, dllDampingRatio=0.5, pllNoiseBandwidth=18.0, dllNoiseBandwidth=3.0))
LOOPS_DEFAULT_RUN = dict(ms=120, T=10, P=40, H=100)        # the quarter chip at 38.192 Msps: 9.3 samples, edges [3, 11]

# 10. BESIDE CANCELLATION: the trio of 400 ms in a DeviceFile at file offset 4096, channel 0 moved; ms = 110, T = 20.
CANCEL_OFF = 4096
CANCEL_RUN = dict(ms=110, T=20, P=40, H=100)
