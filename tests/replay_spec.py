"""numpy restatement of the multi-correlator replay (include/sgx.h, sgx_replay_state / sgx_track_replay): the contract the
host recurrence of csrc/sgx_core.cpp and the HIP kernel of csrc/sgx_replay.hip are tested against.  Test infrastructure
only; the package never imports it.

A tracked channel has, per block k, the rows absoluteSample[k], codeFreq[k], carrFreq[k] of its tracking result.  Block
k's state is rebuilt exactly as the reference forms it (tracking.py:148-251, oracle.track):

    code_freq_k = codeFreq[k-1]  (k = 0: codeFreqBasis)      carr_freq_k = carrFreq[k-1]  (k = 0: acquiredFreq)
    step = code_freq_k / fs      blk = ceil((codeLength - rem_code) / step)
    pos_k = absoluteSample[k-1]  (k = 0: skipNumberOfBytes + codePhase), a BYTE position in the file
    arg = carr_freq_k * 2.0 * pi * (arange(blk + 1) / fs) + rem_carr
    after the block:  rem_code = tp[blk-1] + step - 1023.0  with tp = linspace(rem_code, blk*step + rem_code, blk, False)
                      rem_carr = arg[blk] % (2 pi)

and pos_k + blk * itemsize must equal absoluteSample[k] (ValueError otherwise: the series is not a tracking result of this
record; IndexError when the block ends beyond the record).  For tap offset d_j (chips) and block k < ms_done:

    t = linspace(rem_code + d_j, blk*step + rem_code + d_j, blk, endpoint=False)
    chip = code[(ceil(t) - 1) mod 1023]
    I[j][k] = sum(chip * sin(arg_n) * x_n)      Q[j][k] = sum(chip * cos(arg_n) * x_n)

so d = -dllCorrelatorSpacing, 0, +dllCorrelatorSpacing are the reference's early, prompt and late arms.  Blocks
k >= ms_done hold 0.
"""
import numpy as np

from oracle import softgnss_oracle as orc

STATE_FIELDS = ("blk", "start", "rem_code", "rem_carr", "step", "carr_freq")


def replay(s, record, data_type, prn, acquired_freq, code_phase, absolute_sample, code_freq, carr_freq, ms_done, taps,
           correlate=True):
    """One channel.  record: the file from byte 0 (any array; its bytes are used); data_type: numpy dtype of the samples.
    Returns (I[K][ms], Q[K][ms], state) with state a dict of the STATE_FIELDS arrays [ms] (entries k >= ms_done are 0).
    correlate=False: the state only; the record may then be given as its length in bytes, an int - no byte of it is read."""
    dt = np.dtype(data_type)
    isz = dt.itemsize
    if isinstance(record, (int, np.integer)):
        if correlate:
            raise ValueError("a record given as its length cannot be correlated")
        rec, rec_size = None, int(record)
    else:
        rec = np.ascontiguousarray(record).view(np.uint8).ravel()
        rec_size = rec.size
    fs = s.samplingFreq
    ms = len(absolute_sample)
    taps = [float(d) for d in taps]
    code = orc.generate_ca_code(int(prn) - 1)
    I = np.zeros((len(taps), ms))
    Q = np.zeros((len(taps), ms))
    st = dict(blk=np.zeros(ms, np.int64), start=np.zeros(ms, np.int64), rem_code=np.zeros(ms), rem_carr=np.zeros(ms),
              step=np.zeros(ms), carr_freq=np.zeros(ms))
    pos = int(s.skipNumberOfBytes + code_phase)
    cf = s.codeFreqBasis
    kf = float(acquired_freq)
    rem_code = 0.0
    rem_carr = 0.0
    for k in range(int(ms_done)):
        step = cf / fs
        blk = int(np.ceil((s.codeLength - rem_code) / step))
        if pos + blk * isz != int(absolute_sample[k]):
            raise ValueError("block %d: rebuilt end %d, absoluteSample %d" % (k, pos + blk * isz, int(absolute_sample[k])))
        if pos < 0 or pos + blk * isz > rec_size:
            raise IndexError("block %d ends beyond the record" % k)
        st["blk"][k], st["start"][k], st["rem_code"][k], st["rem_carr"][k] = blk, pos, rem_code, rem_carr
        st["step"][k], st["carr_freq"][k] = step, kf
        arg = kf * 2.0 * np.pi * (np.arange(0, blk + 1) / fs) + rem_carr
        if correlate:
            raw = np.frombuffer(rec[pos:pos + blk * isz].tobytes(), dtype=dt)
            ibb = np.sin(arg[:blk]) * raw
            qbb = np.cos(arg[:blk]) * raw
            for j, d in enumerate(taps):
                t = np.linspace(rem_code + d, blk * step + rem_code + d, blk, endpoint=False)
                chip = code[(np.ceil(t).astype(np.int64) - 1) % 1023]
                I[j, k] = (chip * ibb).sum()
                Q[j, k] = (chip * qbb).sum()
        tp_last = np.linspace(rem_code, blk * step + rem_code, blk, endpoint=False)[blk - 1]
        rem_code = tp_last + step - 1023.0
        rem_carr = arg[blk] % (2 * np.pi)
        pos += blk * isz
        cf = float(code_freq[k])
        kf = float(carr_freq[k])
    return I, Q, st


def replay_channels(s, record, data_type, chans, series, ms_done, taps, correlate=True):
    """chans: (prn, acquiredFreq, codePhase) per channel (prn 0: off); series [n_ch][13][ms] in the order of
    sgx_track_ex.  Returns out[n_ch][K][2][ms] (I then Q, the layout of sgx_track_replay) and the list of states."""
    series = np.asarray(series)
    n_ch, _, ms = series.shape
    out = np.zeros((n_ch, len(taps), 2, ms))
    states = []
    for c, (prn, f, cp) in enumerate(chans):
        if int(prn) == 0:
            states.append(None)
            continue
        done = ms if ms_done is None else int(ms_done[c])
        i, q, st = replay(s, record, data_type, prn, f, cp, series[c, 0], series[c, 1], series[c, 2], done, taps, correlate)
        out[c, :, 0], out[c, :, 1] = i, q
        states.append(st)
    return out, states


def bar(i_p, q_p):
    """The project's bar for correlator series (tests/test_gpu_parity.py): 1e-6 max(1, RMS sqrt(I_P^2 + Q_P^2))."""
    return 1e-6 * max(1.0, float(np.sqrt(np.mean(np.asarray(i_p) ** 2 + np.asarray(q_p) ** 2))))
