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

Five cases need no tracking: sgx_replay_state takes any series whose absoluteSample row obeys its own recurrence, so
handmade() puts blocks wherever a case wants them and the amplitudes are given, not designed.  Their records are random bytes
within +-60, their amplitudes non-integer reals.
  ch32         the limit: 32 channels (PRN 1 .. 32) x 4 blocks at 2.046 Msps, the code phases spread over one code period, so
               that all 32 cover the samples in the middle; 64 KB of code tables in LDS beside the static words
  ch31         the same without the last row, one step under the limit: tells a launch limit from an arithmetic fault
  short_blocks one channel whose recorded code rates are 140 to 400 x 1.023 MHz: behind its first block come 39 blocks of 5 to
               15 samples, across a tile's first sample, at least 20 of them wholly inside one lane's 16 samples (a lane walks
               through several blocks); a second, ordinary channel runs over the same samples
  residues     two channels whose code rates lie a few hundred Hz either side of nominal, blocks of 2045 to 2047 samples: the
               block starts of channel 0, modulo 16, take all 16 values (0: the block before ends on a lane's last sample),
               one lane holds a boundary of both channels, and the record ends exactly with the last block's last sample, at
               a length that is no multiple of 16
  far_offset   the first 5 blocks of the rate2 channels in a window of three tiles less 7 samples, the file 2^33 longer in
               front: rec_file_offset = 2^33 + 5, code phases and absoluteSample beyond 2^33.  Its expectation is the contract
               on the same channels with all three reduced by 2^33 (the recurrence adds integers below 2^53: the states are
               equal apart from `start`)
"""
import functools

import numpy as np

import cancel_spec as spec
import nearfar_scene as nf
from conftest import pkg
from oracle import softgnss_oracle as orc

TILE = 4096
LANE = 16
FAR = 1 << 33
NAMES = ("nearfar", "rate2", "on_tile", "from_start", "rate38", "one_short", "off_done", "clip",
         "ch32", "ch31", "short_blocks", "residues", "far_offset")


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


def _case(s, x, off, chans, series, ms_done=None, gain=1.0, amp=None, near=None):
    """amp None: designed from the prompt sums.  near: (off, chans, series) of the same case moved to the front of the file,
    where its expectation is computed (far_offset)."""
    st = spec.states(s, len(x), off, chans, series, ms_done)
    amp = gain * spec.design(series, st, ms_done, 1) if amp is None else np.array(amp, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.int8)
    for a in (x, series, amp):
        a.setflags(write=False)
    return dict(s=s, x=x, off=int(off), chans=chans, series=series, ms_done=ms_done, amp=amp, states=st, near=near)


def handmade(s, code_phase, acquired_freq, code_freq, carr_freq):
    """A [13][ms] series that sgx_replay_state accepts for a channel started at (acquired_freq, code_phase): rows 1 and 2
    are the given codeFreq and carrFreq, row 0 (absoluteSample) follows from them by the recurrence of replay_spec.replay in
    its own order of operations.  The other rows are 0 - a case passes its amplitudes directly - and acquired_freq, which
    enters no block length, is taken only so that a channel is described in one place."""
    code_freq = np.asarray(code_freq, dtype=np.float64).ravel()
    carr_freq = np.asarray(carr_freq, dtype=np.float64).ravel()
    ms = code_freq.size
    assert carr_freq.size == ms and np.isfinite(float(acquired_freq))
    series = np.zeros((13, ms))
    series[1], series[2] = code_freq, carr_freq
    fs = s.samplingFreq
    pos = int(s.skipNumberOfBytes + code_phase)
    cf = s.codeFreqBasis
    rem_code = 0.0
    for k in range(ms):
        step = cf / fs
        blk = int(np.ceil((s.codeLength - rem_code) / step))
        tp_last = np.linspace(rem_code, blk * step + rem_code, blk, endpoint=False)[blk - 1]
        rem_code = tp_last + step - 1023.0
        pos += blk
        series[0, k] = pos
        cf = float(code_freq[k])
    return series


LOW_FS, LOW_IF, CHIP_RATE = 2.046e6, 0.4e6, 1.023e6


def handmade_case(seed, channels, ms, amp_max, length=None, ms_done=None, off=0):
    """channels: (prn, doppler, code phase, codeFreq[ms]) each; carrFreq wanders a few Hz around IF + doppler.  length: the
    record's (None: to the last block's last sample)."""
    rng = np.random.default_rng(seed)
    s = orc.OracleSettings(samplingFreq=LOW_FS, IF=LOW_IF, numberOfChannels=len(channels), msToProcess=float(ms))
    chans = [(int(p), float(LOW_IF + d), float(cp)) for p, d, cp, _ in channels]
    series = np.stack([handmade(s, cp, f, cf, f + rng.uniform(-20.0, 20.0, ms)) for (p, f, cp), (_, _, _, cf)
                       in zip(chans, channels)])
    done = None if ms_done is None else np.array(ms_done, dtype=np.int32)
    end = _last_end(series, done)
    n = end - off if length is None else int(length)
    x = rng.integers(-60, 61, n).astype(np.int8)
    amp = rng.uniform(-amp_max, amp_max, (len(channels), ms, 2))
    return _case(s, x, off, chans, series, done, amp=amp)


def _ch(n_ch):
    rng = np.random.default_rng(0xC32)
    rows = [(c + 1, float(rng.integers(-4000, 4001)), 3 + 64 * c, CHIP_RATE + rng.uniform(-3.0, 3.0, 4)) for c in range(32)]
    rows = rows[:n_ch]
    last = max(r[2] for r in rows) + 4 * 2046 + 37           # (every block is within a sample of 2046)
    return handmade_case(0xC32, rows, 4, 6.0, length=last)


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
    if name in ("ch32", "ch31"):
        return _ch(int(name[2:]))
    if name == "short_blocks":
        rng = np.random.default_rng(SHORT_SEED)
        fast = CHIP_RATE * rng.uniform(140.0, 400.0, 40)     # codeFreq[k] is the rate of block k + 1: block 0 is ordinary
        start = TILE - 2046 - 150                            # the short blocks run across the first sample of tile 1
        rows = [(13, 1200.0, start, fast), (27, -2600.0, 40, CHIP_RATE + rng.uniform(-3.0, 3.0, 40))]
        return handmade_case(SHORT_SEED, rows, 40, 25.0, length=40 + 3 * 2046 + 21, ms_done=[40, 3])
    if name == "residues":
        rng = np.random.default_rng(RESIDUE_SEED)
        rows = [(6, 3100.0, 16 * 9, CHIP_RATE + rng.uniform(-600.0, 600.0, 40)),
                (18, -900.0, 16 * 9 + 5, CHIP_RATE + rng.uniform(-600.0, 600.0, 40))]
        return handmade_case(RESIDUE_SEED, rows, 40, 25.0)
    if name == "far_offset":
        s, rec, chans, series = _rate2()
        series = np.array(series[:, :, :5])
        off = 5
        x = rec[off:off + 3 * TILE - 7]
        assert _last_end(series) <= off + len(x)
        far_chans = [(p, f, cp + FAR) for p, f, cp in chans]
        far_series = np.array(series)
        far_series[:, 0] += FAR
        assert np.array_equal(far_series[:, 0] - FAR, series[:, 0])                  # (exact in float64)
        return _case(s, x, off + FAR, far_chans, far_series, near=(off, chans, series))
    raise KeyError(name)


SHORT_SEED, RESIDUE_SEED = 2, 1      # (seeds at which the table has the properties test_the_table_covers_what_it_says reads off)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(y, v, clipped, covered) of the contract for the case; computed once."""
    c = get(name)
    off, chans, series = c["near"] or (c["off"], c["chans"], c["series"])
    out = spec.cancel(c["s"], c["x"], off, chans, series, c["ms_done"], c["amp"])
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def compare(name, y, clipped):
    """The comparison rule: y equals the contract's bytes at every sample whose v lies farther than 1e-6 from a half-integer
    and differs by at most 1 at the others; those are at most 1e-4 of the case's samples and none of them lies within 1e-6
    of +-127.5, so the clip count is compared exactly.  Returns the number of excluded samples."""
    return compare_to(expected(name), name, y, clipped)


def compare_to(contract, name, y, clipped=None):
    """The rule of compare() against any result of cancel_spec.cancel (a window of a long record: tests/big_record.py).
    clipped None: the count is the caller's to compare."""
    want, v, want_clipped, covered = contract
    clipped = want_clipped if clipped is None else clipped
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
