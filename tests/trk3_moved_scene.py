"""The scene of the moved-block tests of the speculative tracking kernel (csrc/sgx_trk3.hip), the numpy restatement of the
kernel's block predictor, and the classes of blocks the final pass finds somewhere else than its pass had put them.

The pass of block k + 2 runs with the geometry that block k's start, code phase and length give when they are moved on
TWICE with block k's own code rate (`advance` in t3_map_role).  The final pass of block k + 2 then sees the true start and
length: a block that starts a sample early or late, is a sample shorter or longer, both, or starts in another 16-byte
window of the record than predicted.  The scene makes all of these happen often in 300 code periods: eight hand-given
channels (no acquisition) with code Doppler of both signs - a block a sample shorter or longer than 38 192 every few
blocks - at a signal level whose DLL noise moves that block from where the older rate put it, four of them starting 0, 1, 14
and 15 bytes into a 16-byte window so that moved starts cross windows, the rest mid-window.

Shared by tests/test_trk3_moved_blocks_host.py (the oracle alone) and tests/test_trk3_moved_blocks_gpu.py with its child
process tests/trk3_moved_child.py.  Deterministic; numpy, the package's host generator and the oracle only."""
import os

import numpy as np

MS = 300
FS = 38192000.0
IF = 9548000.0
SEED = 0x7A3B0B6
PRNS = (2, 5, 9, 13, 17, 21, 26, 30)
# Hz: code Doppler +-3 .. 4 Hz; the starts of channels 0 and 1 move DOWN through a window's first byte, those of 2 and 3 up
DOPPLER = (6300.0, 5900.0, -6100.0, -6400.0, 4700.0, -5600.0, 5100.0, -4500.0)
# first sample of a code period, = the channel's codePhase: start & 15 is 0, 1, 14, 15, then mid-window
CODE_START = (12352, 30001, 5006, 20015, 776 + 7, 38000 + 9, 15000 + 6, 9000 + 4)
AMP = (3, 3, 3, 3, 3, 3, 3, 3)     # against a noise sigma of 20: prompt sums of 43 000 with 4 500 rms in quadrature
FREQ_OFF = (3.0, -7.0, 11.0, -2.0, 6.0, -12.0, 1.0, -5.0)                          # Hz the hand-given carrier is off by
CLASSES = ("start-1", "start+1", "length-1", "length+1", "both", "window")
MIN_PER_CLASS = 3


def scene(synth):
    return synth.Scene.make(SEED, FS, IF, PRNS, DOPPLER, CODE_START, AMP)


def channels():
    """[(PRN, acquiredFreq, codePhase)]: what ctx.track and the oracle are given."""
    return [(int(p), IF + d + o, float(c)) for p, d, o, c in zip(PRNS, DOPPLER, FREQ_OFF, CODE_START)]


def record(synth):
    """The int8 record: 300 blocks, the longest of them and every 16-byte load of the last one inside it."""
    return synth.generate(scene(synth), synth.record_length(int(FS / 1000), MS))


def block_table(series, code_phase, fs=FS, basis=1.023e6):
    """(start, length, step, rem) of every block from one channel's series [13, ms]: a block's start is the position the
    block before it ended on (absoluteSample), its code rate the one the block before it left (codeFreq), its code phase
    carried as tracking.py:190 carries it (the last prompt ramp value + step - 1023)."""
    ms = series.shape[1]
    end = series[0].astype(np.int64)
    start = np.r_[np.int64(code_phase), end[:-1]]
    blk = end - start
    step = np.r_[basis, series[1][:-1]] / fs
    rem = np.zeros(ms)
    for k in range(ms - 1):
        b = int(blk[k])
        assert b == int(np.ceil((1023.0 - rem[k]) / step[k])), (k, b)          # (the series' own lengths: tracking.py:148)
        tp = np.linspace(rem[k], b * step[k] + rem[k], b, endpoint=False)
        rem[k + 1] = tp[b - 1] + step[k] - 1023.0
    return start, blk, step, rem


def advance(pos, rem, blk, step):
    """t3_map_role's `advance`: the block behind (pos, rem, blk) when the code rate stays what it is."""
    pos = pos + blk
    rem = blk * step + rem - 1023.0
    nb = int(np.ceil((1023.0 - rem) / step))
    return pos, rem, max(nb, 1)


def predicted(start, blk, step, rem):
    """(start, length) the pass of every block k >= 2 ran with: two `advance` steps from block k - 2 with that block's rate
    (blocks 0 and 1 have passes of their own - block 0's rates, on the chain's first barrier - and are left out: -1)."""
    ms = len(start)
    ps, pl = -np.ones(ms, np.int64), -np.ones(ms, np.int64)
    for k in range(ms - 2):
        p, r, b = int(start[k]), float(rem[k]), int(blk[k])
        p, r, b = advance(p, r, b, float(step[k]))
        p, r, b = advance(p, r, b, float(step[k]))
        ps[k + 2], pl[k + 2] = p, b
    return ps, pl


def classes(series, code_phase):
    """{class: [block numbers]} of one channel (blocks 2 .. MS - 1; a block may be in `window` and in another class)."""
    start, blk, step, rem = block_table(series, code_phase)
    ps, pl = predicted(start, blk, step, rem)
    out = {c: [] for c in CLASSES}
    for k in range(2, len(start)):
        ds, dl = int(start[k] - ps[k]), int(blk[k] - pl[k])
        if ds == -1 and dl == 0:
            out["start-1"].append(k)
        if ds == 1 and dl == 0:
            out["start+1"].append(k)
        if ds == 0 and dl == -1:
            out["length-1"].append(k)
        if ds == 0 and dl == 1:
            out["length+1"].append(k)
        if ds != 0 and dl != 0:
            out["both"].append(k)
        if (int(start[k]) ^ int(ps[k])) & ~15:
            out["window"].append(k)
    return out


def class_counts(all_series):
    """{class: [blocks of set 0 (even), blocks of set 1 (odd)]} over the scene's channels."""
    n = {c: [0, 0] for c in CLASSES}
    for ch, (_, _, phase) in enumerate(channels()):
        for c, ks in classes(all_series[ch], phase).items():
            for k in ks:
                n[c][k & 1] += 1
    return n


_ORACLE = {}


def oracle_series(synth, rec=None):
    """[8, 13, MS]: the numpy restatement of the reference's track() on the scene's record, computed once per process."""
    if "s" not in _ORACLE:
        import concurrent.futures
        from oracle_helpers import oracle_channel
        host = record(synth) if rec is None else rec
        args = [(host, p, f, c, MS) for p, f, c in channels()]
        with concurrent.futures.ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            s = np.stack(list(ex.map(oracle_channel, args)))
        s.setflags(write=False)
        _ORACLE["s"] = s
    return _ORACLE["s"]
