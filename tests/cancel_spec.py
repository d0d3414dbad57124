"""numpy statement of the strong-signal cancellation (include/sgx.h: sgx_cancel_design, sgx_if_cancel, sgx_cancel_host): the
contract the host twin of csrc/sgx_cancel.cpp and the HIP kernel of csrc/sgx_cancel.hip are tested against.  Test
infrastructure only; the package never imports it.

A tracked channel's blocks are those of tests/replay_spec.py: block k of channel c has the state (start, blk, rem_code,
rem_carr, step, carr_freq) of replay_spec.replay(..., correlate=False).  With an amplitude pair (aI, aQ) per block, sample
i < blk of block k < ms_done[c] is rebuilt as

    arg_i  = carr_freq * 2.0 * pi * (i / fs) + rem_carr
    t_i    = linspace(rem_code, blk*step + rem_code, blk, endpoint=False)[i]
    chip_i = code[(ceil(t_i) - 1) mod 1023]
    s_c    = chip_i * (aI * sin(arg_i) + aQ * cos(arg_i))

at file position n = start + i, and v[n] = x[n] - sum_c s_c[n], the channels subtracted in channel order.  Where at least one
block covers n, y[n] = clip(rint(v[n]), -127, 127) (round half to even; the rails of every other stage); elsewhere y[n] =
x[n], so a byte of -128 that no block covers stays -128.  The clip count is the number of covered samples whose rint(v) lay
outside [-127, 127].

design(): the amplitude pairs from the prompt sums.  p_j = 2 (I_P, Q_P)[j] / blk_j is what a signal of s_c's form leaves in
the prompt arm.  (aI, aQ)_k is the mean - added in ascending j - of d p_j over the blocks j < ms_done with
|j - k| <= (smooth - 1) / 2, d = sign(pI_j pI_k + pQ_j pQ_k) with 0 counting as +1: the data-bit sign of block j against
block k.  smooth is odd, 1 .. 41.
"""
import numpy as np

import replay_spec
from oracle import softgnss_oracle as orc

MAX_CHANNELS = 32
MAX_SMOOTH = 41
HALF_MARGIN = 1e-6       # a sample whose v lies this close to a half-integer is a rounding decision


def states(s, record_bytes, rec_file_offset, chans, series, ms_done):
    """The block state of every channel (None for a channel that is off), the record being bytes [rec_file_offset,
    rec_file_offset + record_bytes) of the file: replay_spec's recurrence on the file's length alone - no byte is read, so
    no image is made, and an offset beyond 2^33 costs nothing."""
    series = np.asarray(series)
    n_ch, _, ms = series.shape
    image = int(rec_file_offset) + int(record_bytes)
    out = []
    for c, (prn, f, cp) in enumerate(chans):
        if int(prn) == 0:
            out.append(None)
            continue
        done = ms if ms_done is None else int(ms_done[c])
        st = replay_spec.replay(s, image, "int8", prn, f, cp, series[c, 0], series[c, 1], series[c, 2], done, (0.0,),
                                correlate=False)[2]
        if done and int(st["start"][0]) < int(rec_file_offset):
            raise IndexError("channel %d starts before the record" % c)
        out.append(st)
    return out


def design(series, state, ms_done=None, smooth=1):
    """amp[n_ch][ms][2] from series [n_ch][13][ms] and the list of states (None: a channel that is off)."""
    series = np.asarray(series, dtype=np.float64)
    n_ch, _, ms = series.shape
    smooth = int(smooth)
    if not (1 <= smooth <= MAX_SMOOTH and smooth % 2 == 1):
        raise ValueError("smooth is odd, 1 .. %d" % MAX_SMOOTH)
    half = (smooth - 1) // 2
    amp = np.zeros((n_ch, ms, 2))
    for c in range(n_ch):
        if state[c] is None:
            continue
        done = ms if ms_done is None else int(ms_done[c])
        blk = state[c]["blk"][:done].astype(np.float64)
        p_i = 2.0 * series[c, 3, :done] / blk
        p_q = 2.0 * series[c, 7, :done] / blk
        for k in range(done):
            lo, hi = max(0, k - half), min(done - 1, k + half)
            s_i = s_q = 0.0
            for j in range(lo, hi + 1):
                d = -1.0 if p_i[j] * p_i[k] + p_q[j] * p_q[k] < 0.0 else 1.0
                s_i = s_i + d * p_i[j]
                s_q = s_q + d * p_q[j]
            amp[c, k, 0] = s_i / float(hi - lo + 1)
            amp[c, k, 1] = s_q / float(hi - lo + 1)
    return amp


def cancel(s, record, rec_file_offset, chans, series, ms_done, amp):
    """record: int8, bytes [rec_file_offset, rec_file_offset + len(record)) of the file.  Returns (y int8, v float64,
    clipped, covered bool)."""
    x = np.ascontiguousarray(record, dtype=np.int8).ravel()
    series = np.asarray(series, dtype=np.float64)
    amp = np.asarray(amp, dtype=np.float64)
    n_ch, _, ms = series.shape
    if not 1 <= n_ch <= MAX_CHANNELS:
        raise ValueError("1 .. %d channels" % MAX_CHANNELS)
    if amp.shape != (n_ch, ms, 2) or not np.all(np.isfinite(amp)):
        raise ValueError("amp is finite float64[n_ch][ms][2]")
    fs = s.samplingFreq
    st = states(s, x.size, rec_file_offset, chans, series, ms_done)
    v = x.astype(np.float64)
    covered = np.zeros(x.size, dtype=bool)
    for c in range(n_ch):
        if st[c] is None:
            continue
        code = orc.generate_ca_code(int(chans[c][0]) - 1)
        done = ms if ms_done is None else int(ms_done[c])
        for k in range(done):
            blk, step = int(st[c]["blk"][k]), st[c]["step"][k]
            rem_code, rem_carr, kf = st[c]["rem_code"][k], st[c]["rem_carr"][k], st[c]["carr_freq"][k]
            p0 = int(st[c]["start"][k]) - int(rec_file_offset)
            arg = kf * 2.0 * np.pi * (np.arange(0, blk) / fs) + rem_carr
            t = np.linspace(rem_code, blk * step + rem_code, blk, endpoint=False)
            chip = code[(np.ceil(t).astype(np.int64) - 1) % 1023]
            sc = chip * (amp[c, k, 0] * np.sin(arg) + amp[c, k, 1] * np.cos(arg))
            v[p0:p0 + blk] = v[p0:p0 + blk] - sc
            covered[p0:p0 + blk] = True
    r = np.rint(v)
    clip = covered & ((r > 127.0) | (r < -127.0))
    y = np.where(covered, np.clip(r, -127.0, 127.0), x).astype(np.int8)
    return y, v, int(clip.sum()), covered


def decisions(v, covered, margin=HALF_MARGIN):
    """The covered samples whose v lies within `margin` of a half-integer: where two correct implementations may round to
    neighbouring integers."""
    frac = np.abs(v - np.floor(v) - 0.5)
    return covered & (frac <= margin)
