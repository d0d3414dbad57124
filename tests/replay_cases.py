"""The reference-anchored cases of the multi-correlator replay, shared by tests/test_replay_host.py and
tests/test_replay_gpu.py: each is (oracle settings, record, numpy dtype, channels, golden series), the records built as
tests/test_oracle_golden.py builds them.  Test infrastructure only."""
import numpy as np

from conftest import load_golden, pkg, scene_from_json
from oracle import softgnss_oracle as orc

# rows of the [13][ms] series: the early, prompt and late arms are the taps (-spacing, 0, +spacing)
I_ROWS = (4, 3, 5)      # I_E I_P I_L
Q_ROWS = (6, 7, 8)      # Q_E Q_P Q_L


def chans_of(prn, freq, cph):
    return [(int(p), float(f), float(c)) for p, f, c in zip(prn, freq, cph)]


def case_default(default_record):
    g = load_golden("trk_default.npz")
    s = orc.OracleSettings(numberOfChannels=4, msToProcess=float(g["ms"]))
    return s, default_record, "int8", chans_of(g["ch_PRN"], g["ch_acquiredFreq"], g["ch_codePhase"]), g["series"]


def case_rate2():
    g = load_golden("rate2.npz")
    s = orc.OracleSettings(samplingFreq=16367600.0, IF=4130400.0, msToProcess=float(g["ms"]), numberOfChannels=3)
    rec = pkg("synth").generate(scene_from_json(g["scene"]), int(g["n_samples"]))
    return s, rec, "int8", chans_of(g["ch_PRN"], g["ch_acquiredFreq"], g["ch_codePhase"]), g["series"]


def cases_int16():
    g = load_golden("trk_int16.npz")
    rec16 = (pkg("synth").generate(scene_from_json(g["scene"]), int(g["n_samples"])).astype(np.int16) * int(g["scale"])).astype("<i2")
    out = []
    for case in ("locked", "as_is"):
        nch = len(g[case + "_PRN"])
        s = orc.OracleSettings(numberOfChannels=nch, msToProcess=float(g["ms"]), dataType='int16',
                               skipNumberOfBytes=int(g[case + "_skip"]))
        out.append((s, rec16, "<i2", chans_of(g[case + "_PRN"], g[case + "_acquiredFreq"], g[case + "_codePhase"]),
                    g[case + "_series"]))
    return out


def arms(series):
    """[n_ch][3][2][ms] in the layout of sgx_track_replay from the golden series' six correlator rows."""
    series = np.asarray(series)
    return np.stack([np.stack([series[:, i] for i in I_ROWS], axis=1), np.stack([series[:, q] for q in Q_ROWS], axis=1)], axis=2)


def noiseless_record(s, ms, prn=7, amp=60, doppler=1234.0, cp0=5000):
    """One satellite, no noise, int8 (the generator of synth.py always adds noise): chips at the Doppler-scaled chip rate
    from sample cp0, carrier at IF + doppler."""
    fs = s.samplingFreq
    code = orc.generate_ca_code(prn - 1)
    n = np.arange(s.samplesPerCode * (ms + 2))
    t = (n - cp0) * (1.023e6 * (1 + doppler / 1575.42e6)) / fs
    chip = code[np.floor(t).astype(np.int64) % 1023]
    rec = np.round(amp * chip * np.cos(2 * np.pi * (s.IF + doppler) * n / fs + 0.3)).astype(np.int8)
    ch = dict(PRN=np.array([prn]), acquiredFreq=np.array([s.IF + doppler + 40.0]), codePhase=np.array([float(cp0)]), status=['T'])
    return rec, ch
