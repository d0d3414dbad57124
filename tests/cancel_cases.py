"""The case table of the strong-signal cancellation, shared by tests/test_cancel_host.py and tests/test_cancel_gpu.py.  A case
is a dict: s (oracle settings), x (the int8 record), off (the file offset of its first byte), chans, series [n_ch][13][ms],
ms_done (or None), amp [n_ch][ms][2].  The series are the oracle's tracking of a synthetic record, 4 to 40 blocks; a case
is built once and its contract result (cancel_spec.cancel) computed once, and neither is written to afterwards.

The kernel's tile is 4096 samples, a lane's share 16 (csrc/sgx_cancel.hip).  The table covers:
  nearfar      the scene of tests/nearfar_scene.py: 2 channels x 40 blocks at 16.368 Msps, the record from file offset 0
  rate2        2.046 Msps, 3 channels x 12 blocks: two or three block boundaries of every channel in each tile
  on_tile      the same channels in a window of the file, at a file offset chosen so that block 3 of channel 0 starts exactly
               on a tile's first sample (and, the blocks being contiguous, block 2 ends there)
  from_start   4.092 Msps, the record a window that begins exactly at the first sample of channel 0 (record index 0) and ends
               inside a tile, 5 samples behind the last block
  rate38       38.192 Msps, the default scene's 8 channels x 4 blocks
  one_short    one channel, ms_done 1 of 4, in a record of 3000 samples: shorter than a tile
  off_done     4 channel rows of which one has prn == 0, one ms_done == 0 and one ms_done < ms; bytes of -128 in front of the
               first block (they stay) and inside the blocks (they clip); the record ends inside a tile and inside a lane
  clip         the rate2 channels at ten times their amplitudes: thousands of outputs on the rails
"""
import functools

import numpy as np

import cancel_spec as spec
import nearfar_scene as nf
from conftest import pkg
from oracle import softgnss_oracle as orc

TILE = 4096
NAMES = ("nearfar", "rate2", "on_tile", "from_start", "rate38", "one_short", "off_done", "clip")


def _tracked(fs, IF, prns, dopplers, starts, amps, ms, seed):
    """(settings, file image, chans, series) of a synthetic record tracked by the oracle from the true code starts."""
    synth = pkg("synth")
    s = orc.OracleSettings(samplingFreq=fs, IF=IF, numberOfChannels=len(prns), msToProcess=float(ms))
    scene = synth.Scene.make(seed, fs=fs, IF=IF, prns=prns, dopplers=dopplers, code_starts=starts, amps=amps)
    rec = synth.generate(scene, synth.record_length(s.samplesPerCode, ms) + max(starts))
    chans = [(int(p), float(IF + d), float(c)) for p, d, c in zip(prns, dopplers, starts)]
    ch = dict(PRN=np.array(prns), acquiredFreq=np.array([c[1] for c in chans]), codePhase=np.array([c[2] for c in chans]),
              status=['T'] * len(prns))
    return s, rec, chans, orc.stack_series(orc.track(s, ch, rec, ms=ms))


def _case(s, x, off, chans, series, ms_done=None, gain=1.0):
    st = spec.states(s, len(x), off, chans, series, ms_done)
    amp = gain * spec.design(series, st, ms_done, 1)
    x = np.ascontiguousarray(x, dtype=np.int8)
    for a in (x, series, amp):
        a.setflags(write=False)
    return dict(s=s, x=x, off=int(off), chans=chans, series=series, ms_done=ms_done, amp=amp, states=st)


@functools.lru_cache(maxsize=None)
def _rate2():
    return _tracked(2.046e6, 0.4e6, [5, 9, 21], [700, -1500, 2400], [100, 1500, 777], [20, 12, 9], 12, 0xC0DE)


def _last_end(series, ms_done=None):
    ends = [series[c, 0, (series.shape[2] if ms_done is None else ms_done[c]) - 1] for c in range(series.shape[0])
            if ms_done is None or ms_done[c] > 0]
    return int(max(ends))


@functools.lru_cache(maxsize=None)
def get(name):
    if name == "nearfar":
        s, rec, _, chans, series = nf.oracle_run()
        return _case(s, rec, 0, chans, series)
    if name in ("rate2", "clip"):
        s, rec, chans, series = _rate2()
        return _case(s, rec, 0, chans, series, gain=10.0 if name == "clip" else 1.0)
    if name == "on_tile":
        s, rec, chans, series = _rate2()
        s = orc.OracleSettings(**vars(s))
        first = min(int(c[2]) for c in chans)
        boundary = int(series[0, 0, 2])                  # where block 2 of channel 0 ends and block 3 starts
        off = boundary - TILE * ((boundary - first) // TILE + 1)
        pad = -off if off < 0 else 0                     # the file grows in front so that the offset is not negative
        if pad:
            rec = np.concatenate((np.zeros(pad, dtype=np.int8), rec))
            series = np.array(series)
            series[:, 0] += pad
            s.skipNumberOfBytes = pad
            off = 0
            boundary += pad
            # a window at a non-zero offset all the same: one tile further into the padded file is still in front of `first`
        assert (boundary - off) % TILE == 0 and off <= first + pad
        return _case(s, rec[off:_last_end(series) + 40], off, chans, series)
    if name == "from_start":
        s, rec, chans, series = _tracked(4.092e6, 1.023e6, [2, 30], [-300, 3300], [4500, 6000], [15, 10], 6, 0xF00D)
        off = 4500
        return _case(s, rec[off:_last_end(series) + 5], off, chans, series)
    if name == "rate38":
        sc = pkg("synth").Scene.default()
        prns = [d["prn"] for d in sc.sats]
        dop = [1250, -3100, 4800, -650, 2900, -4400, 350, -1900]
        starts = [12345, 30001, 5, 20000, 777, 38000, 15000, 9000]
        s, rec, chans, series = _tracked(38.192e6, 9.548e6, prns, dop, starts, [8, 7, 6, 7, 8, 6, 7, 6], 4, 0x5EED0001)
        return _case(s, rec, 0, chans, series)
    if name == "one_short":
        s, rec, chans, series = _tracked(2.046e6, 0.4e6, [17], [-900], [600], [25], 4, 0xAB)
        done = np.array([1], dtype=np.int32)
        assert int(series[0, 0, 0]) - 300 <= 3000
        return _case(s, rec[300:3300], 300, chans, series, done)
    if name == "off_done":
        s, rec, chans, series = _tracked(4.092e6, 1.023e6, [4, 8, 12, 25], [500, -700, 900, -2100], [3000, 5000, 3500, 8000],
                                         [14, 9, 11, 12], 8, 0xD0E)
        chans = [chans[0], (0, 0.0, 0.0), chans[2], chans[3]]
        done = np.array([8, 8, 0, 5], dtype=np.int32)
        x = np.array(rec[:_last_end(series, [8, 0, 0, 5]) + 1003])
        assert x.size % 16 != 0 and x.size % TILE != 0
        x[[0, 17, 2999]] = -128                          # in front of the first block: no block covers them
        x[[3000, 3001, 9000, 20000]] = -128              # inside channel 0's blocks
        return _case(s, x, 0, chans, series, done)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(y, v, clipped, covered) of the contract for the case; computed once."""
    c = get(name)
    out = spec.cancel(c["s"], c["x"], c["off"], c["chans"], c["series"], c["ms_done"], c["amp"])
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def compare(name, y, clipped):
    """The comparison rule: y equals the contract's bytes at every sample whose v lies farther than 1e-6 from a half-integer
    and differs by at most 1 at the others; those are at most 1e-4 of the case's samples and none of them lies within 1e-6
    of +-127.5, so the clip count is compared exactly.  Returns the number of excluded samples."""
    want, v, want_clipped, covered = expected(name)
    y = np.asarray(y)
    assert y.dtype == np.int8 and y.shape == want.shape, (name, y.dtype, y.shape)
    dec = spec.decisions(v, covered)
    assert dec.sum() <= 1e-4 * want.size, (name, int(dec.sum()), want.size)
    assert not np.any(np.abs(np.abs(v[dec]) - 127.5) <= spec.HALF_MARGIN), name
    diff = np.abs(y.astype(np.int16) - want.astype(np.int16))
    bad = np.flatnonzero((diff != 0) & ~dec)
    assert bad.size == 0, (name, bad[:8], y[bad[:8]], want[bad[:8]], v[bad[:8]])
    assert diff.max(initial=0) <= 1, name
    assert int(clipped) == want_clipped, (name, int(clipped), want_clipped)
    return int(dec.sum())
