"""Records longer than 4 GiB: the helpers of tests/test_big_record_host.py (their arithmetic at a small boundary, no GPU) and
tests/test_big_record_gpu.py (every path that reads a record, at positions beyond 2^31 and 2^32).  Test infrastructure; no GPU
code, no product import.

THE RULE EVERY CASE OBEYS: A WRAP MUST BE VISIBLE (wrap_visible).  A window that the GPU test compares must hold bytes that
differ from what the same computation gives with its input positions reduced by the boundary B = 2^32 (an index truncated to
32 bits) and by B / 2 = 2^31 (a signed index that went negative and was clamped or wrapped).  A record of period 2^20 fails it:
2^20 divides both, so a truncated load address reads the same data.  Hence the three kinds of records used here:

  tiled   a random int8 block of P bytes over and over, P = 105 * 2^13 = 860 160: a multiple of every framing unit of the stages
          (16 M for M = 1, 2, 3; 2 * 4 bytes of an I/Q float frame; 16 D for D = 16; whole conditioning blocks) that divides
          neither 2^31 nor 2^32.  The record is `reps` whole blocks and a rest that continues the period.
  scene   the signal at p - 2^32 is another piece of the scene: the generator is a pure function of the position.
  sparse  zeros (128 for uint8) with the signal in the last window: a wrapped read finds the filler.

Everything is written against the boundary B, so that the host test can hold the expectations to brute force at B = 2^16 (or
2^20 where a stage's framing needs a longer block): a stage's window is the contract on the few input bytes it depends on, a
whole-record counter is  first + (reps - 2) middle + last  from the contract on two and on three blocks (see counters)."""
import numpy as np

import cancel_cases
import cancel_spec
import cond_spec
import decim_spec
import iq_spec
import notch_spec
import requant_spec
import resamp_spec
import waterfall_spec
from oracle import softgnss_oracle as orc

B32 = 1 << 32
P32 = 105 << 13
EXTRA32 = 3 * 65536 + 48 * 7          # bytes behind 2^32: a few tiles of every stage, a multiple of 48
SEED = 20321


# ---- the rule -----------------------------------------------------------------------------------------------------------

def shifted(at, by):
    """The record as a reader whose positions came out `by` too small sees it."""
    return lambda a, b: at(a - by, b - by)


def wrap_visible(at, contract, window, B=B32, sparse=False):
    """at(a, b): the record's bytes at positions [a, b), defined for ANY integers (what a wrapped index would find);
    contract(at, w0, w1): the bytes the host expects in the window [w0, w1), every input byte taken through `at`.  Asserts
    that the expectation, the one with input positions reduced by B and the one with them reduced by B / 2 are pairwise
    different, and returns the expectation.  Run on the CPU before anything is compared with the device.  sparse: a record
    of filler with the signal in the window - both wrapped readings find the filler, so only the expectation must differ
    from either."""
    w0, w1 = window
    want = np.asarray(contract(at, w0, w1))
    by_b = np.asarray(contract(shifted(at, B), w0, w1))
    by_half = np.asarray(contract(shifted(at, B // 2), w0, w1))
    assert want.size and want.shape == by_b.shape == by_half.shape, (window, want.shape, by_b.shape, by_half.shape)
    assert want.tobytes() != by_b.tobytes(), "window %r: positions reduced by B give the same bytes" % (window,)
    assert want.tobytes() != by_half.tobytes(), "window %r: positions reduced by B / 2 give the same bytes" % (window,)
    assert sparse or by_b.tobytes() != by_half.tobytes(), "window %r: the two wrapped readings give the same bytes" % (window,)
    return want


def identity(at, w0, w1):
    """The contract of a path that hands the record's bytes on as they are (download, a window given to an oracle)."""
    return at(w0, w1)


# ---- tiled records ------------------------------------------------------------------------------------------------------

class Tiled(object):
    """A random int8 block of P bytes repeated: n = B + extra bytes, `reps` whole blocks and `rest` bytes of one more."""

    def __init__(self, B=B32, P=P32, extra=EXTRA32, seed=SEED, n=None):
        self.B, self.P = int(B), int(P)
        self.block = np.random.default_rng(seed).integers(-128, 128, self.P).astype(np.int8)
        self.block.setflags(write=False)
        self.n = self.B + int(extra) if n is None else int(n)
        self.reps, self.rest = divmod(self.n, self.P)
        assert self.reps >= 3

    def at(self, a, b):
        """Bytes [a, b) of the period, at any integer position."""
        return self.block[np.arange(int(a), int(b), dtype=np.int64) % self.P]

    def build(self):
        """The whole record on the host (the caller uploads it and lets go of it at once)."""
        b = np.empty(self.n, dtype=np.int8)
        b[:self.reps * self.P].reshape(self.reps, self.P)[:] = self.block
        b[self.reps * self.P:] = self.block[:self.rest]
        return b

    def model(self, k):
        """k whole blocks and the rest: the record with reps - k blocks taken out of its middle."""
        return np.concatenate([self.block] * k + [self.block[:self.rest]])

    def head(self, n):
        """The same period cut at n bytes: a record of its own (the resampler's 16 / 1 case)."""
        return Tiled(self.B, self.P, n=n, seed=SEED) if n != self.n else self

    def sums(self, a, b):
        """([count, sum x, sum x^2, sum x^4] as exact Python integers, hist int64[256]) of bytes [a, b), formed from the block
        by multiplication: nothing grows with b - a."""
        v = self.block.astype(np.int64)

        def upto(x):
            q, r = divmod(int(x), self.P)
            return ([q * int((v ** k).sum()) + int((v[:r] ** k).sum()) for k in (1, 2, 4)],
                    q * np.bincount(v + 128, minlength=256) + np.bincount(v[:r] + 128, minlength=256))

        (sa, ha), (sb, hb) = upto(a), upto(b)
        return [int(b) - int(a)] + [y - x for x, y in zip(sa, sb)], (hb - ha).astype(np.int64)


# ---- record stages ------------------------------------------------------------------------------------------------------

class Stage(object):
    """A record stage for window and counter expectations.  num / den: output bytes per input byte; unit: input bytes a chunk
    must start at a multiple of (the stage's framing; unit * num / den is whole); halo: input bytes either side that an
    output depends on.  run(chunk, lo) -> (int8 output of the contract on the record `chunk`, dict of its counters): the
    chunk starts at input byte `lo` of the real record and is treated as a record of its own, zeros outside."""
    name = ""
    num = den = unit = 1
    halo = 0
    width = 16384                     # output bytes of a window of the GPU test: two tiles of the stage's kernel, or more

    def out_len(self, n):
        return -(-int(n) * self.num // self.den)

    def out_of(self, byte):
        """The output index that corresponds to input byte `byte`."""
        return int(byte) * self.num // self.den

    def window(self, at, n, w0, w1):
        """Output bytes [w0, w1) of the stage run on the record of n bytes that `at` reads: the contract on the input bytes
        they depend on, cut at the record's ends only."""
        lo = ((w0 * self.den // self.num) - self.halo) // self.unit * self.unit
        hi = -(-(-(-w1 * self.den // self.num) + self.halo) // self.unit) * self.unit
        lo, hi = max(lo, 0), min(hi, int(n))
        y = self.run(at(lo, hi), lo)[0]
        o0 = lo * self.num // self.den
        assert (lo * self.num) % self.den == 0 and 0 <= w0 - o0 and w1 - o0 <= y.size, (self.name, w0, w1, lo, hi, y.size)
        return y[w0 - o0:w1 - o0]

    def contract(self, n):
        return lambda at, w0, w1: self.window(at, n, w0, w1)

    def windows(self, rec, w=None):
        """The windows of w output bytes the GPU test compares: at the start, across the output indices of input bytes B / 2
        and B, across output indices B / 2 and B themselves (those of them that the output has), at the end."""
        w = self.width if w is None else w
        n_out = self.out_len(rec.n)
        mid = sorted(set(x - w // 2 for b in (rec.B // 2, rec.B) for x in (self.out_of(b), b)))
        return [(0, w)] + [(m, m + w) for m in mid if 0 <= m and m + w <= n_out] + [(n_out - w, n_out)]

    def counters(self, rec):
        """The stage's counters over the whole tiled record as exact integers: with f(k) the contract's counters on k blocks
        and the rest, the middle block is worth f(3) - f(2) (every block between the first and the last sees the same
        bytes either side, the halo being shorter than a block), so the record's are first + (reps - 2) middle + last =
        f(2) + (reps - 2) (f(3) - f(2))."""
        assert self.halo < rec.P and rec.P % self.unit == 0 and (rec.P * self.num) % self.den == 0
        f2, f3 = self.run(rec.model(2), 0)[1], self.run(rec.model(3), 0)[1]
        return dict((k, int(f2[k]) + (rec.reps - 2) * (int(f3[k]) - int(f2[k]))) for k in f2)


def taps_in_bound(rng, n, shift, max_tap=32512):
    """n random int16 taps whose sums land on both sides of the clip at this shift, inside 128 sum|h| < 2^31."""
    budget = (2 ** 31 - 1) // 128
    a = 100.0 * 2.0 ** shift * np.sqrt(3.0) / (74.0 * np.sqrt(n))
    a = int(min(max(a, 1.0), max_tap, 1.6 * budget / n))
    h = rng.integers(-a, a + 1, n)
    assert 128 * int(np.abs(h).sum()) < 2 ** 31
    return h.astype(np.int16)


class Notch(Stage):
    name = "filter_record"
    counters = lambda self, rec: {}

    def __init__(self, L=255, S=14, seed=1):
        self.h, self.S, self.halo = taps_in_bound(np.random.default_rng(seed), L, S), S, (L - 1) // 2

    def run(self, chunk, lo):
        return notch_spec.apply(chunk, self.h, self.S), {}


class IQ(Stage):
    name = "iq_to_if"
    unit = 4
    counters = lambda self, rec: {}

    def __init__(self, L=63, S=14, flags=iq_spec.Q_FIRST | iq_spec.OFFSET_BINARY, seed=2):
        self.h, self.S, self.flags, self.halo = taps_in_bound(np.random.default_rng(seed), L, S), S, flags, (L - 1) // 2 + 1

    def run(self, chunk, lo):
        return iq_spec.convert(chunk, self.h, self.S, self.flags), {}


def requant_counts(b, dtype):
    """n_finite, n_nonfinite and - int16 only - sum and sum_sq of a record's elements, as exact integers."""
    x = requant_spec.elements(b, dtype)
    if x.dtype == requant_spec.INT16:
        v = x.astype(np.int64)
        return dict(n_finite=v.size, n_nonfinite=0, sum=int(v.sum()), sum_sq=int((v * v).sum()))
    ok = np.isfinite(x)
    return dict(n_finite=int(ok.sum()), n_nonfinite=int(x.size - ok.sum()))


class Requant(Stage):
    """requantize and requant_stats of the record read as int16 or float32."""
    name = "requantize"

    def __init__(self, dtype, mult=1, shift=0, scale=1.0):
        self.dtype = np.dtype(dtype)
        self.den = self.unit = self.dtype.itemsize
        self.gain = dict(mult=mult, shift=shift, scale=scale)

    def run(self, chunk, lo):
        y = requant_spec.quantise(chunk, self.dtype, **self.gain)
        c = requant_counts(chunk, self.dtype)
        c["clipped"] = int(np.count_nonzero(np.abs(y.astype(np.int16)) == 127))
        return y, c

    def max_abs(self, rec):
        """The largest finite magnitude of the record: that of one block (a maximum is not a sum)."""
        x = requant_spec.elements(rec.block, self.dtype)
        return float(np.abs(x[np.isfinite(x)].astype(np.float64)).max())


class Cond(Stage):
    """cond_stats and condition: blocks that tile the period, a plan of one period's entries over and over."""
    name = "condition"

    def __init__(self, rec, dtype, lanes, block, blank_q4=44, guard=1):
        self.dtype, self.lanes, self.block, self.blank_q4, self.guard = np.dtype(dtype), lanes, block, blank_q4, guard
        self.den = self.dtype.itemsize
        self.unit = self.halo = block * lanes * self.den                  # a block, in bytes; guard <= 64 frames < a block
        assert rec.P % self.unit == 0
        self.period = rec.P // self.unit                                  # blocks of the period
        self.stats = cond_spec.block_stats(rec.block, self.dtype, lanes, block, blank_q4)
        assert self.stats.size == self.period
        self.plan = cond_spec.plan(self.stats, lanes, blank_q4, 100.0, 4.0)

    def entries(self, k0, K, of):
        return of[(k0 + np.arange(K)) % self.period]

    def run(self, chunk, lo):
        K = -(-chunk.size // self.unit)
        y, blanked, clipped = cond_spec.condition(chunk, self.dtype, self.lanes, self.block,
                                                  self.entries(lo // self.unit, K, self.plan), self.guard)
        return y, dict(blanked=blanked, clipped=clipped)

    def record_plan(self, rec):
        return self.entries(0, -(-rec.n // self.unit), self.plan)

    def record_stats(self, rec):
        """Every block's statistics: the period's, and the contract on the last, partial block."""
        K = -(-rec.n // self.unit)
        out = self.entries(0, K, self.stats).copy()
        if rec.n % self.unit:
            out[K - 1] = cond_spec.block_stats(rec.at((K - 1) * self.unit, rec.n), self.dtype, self.lanes, self.block,
                                               self.blank_q4)[0]
        return out


class Resamp(Stage):
    name = "resample"

    def __init__(self, L, M, n_taps, S=14, seed=3):
        self.num, self.den, self.unit, self.S = L, M, M, S
        self.h = taps_in_bound(np.random.default_rng(seed), n_taps, S + 0.5 * np.log2(L))   # (one tap in L meets a sample)
        self.halo = (n_taps - 1) // 2 // L + 2
        self.width = 8192 * L                                             # (a workgroup makes 65536 L / 16 output bytes)

    def run(self, chunk, lo):
        y, over = resamp_spec.quantise(resamp_spec.sums_phased(resamp_spec.samples(chunk), self.h.astype(np.int64),
                                                               self.num, self.den), self.S)
        return y, dict(clipped=int(np.count_nonzero(over)))


class Decim(Stage):
    name = "decimate"

    def __init__(self, D, L, S=14, seed=4):
        self.den = self.unit = D
        self.S, self.halo = S, (L - 1) // 2 + D
        self.h = taps_in_bound(np.random.default_rng(seed), L, S)

    def run(self, chunk, lo):
        y, over = decim_spec.quantise(decim_spec.sums(chunk, self.h, 1, self.den), self.S)
        return y, dict(clipped=int(np.count_nonzero(over)))


def stage_cases(rec, small=False):
    """name -> (stage, the tiled record it reads) of the GPU test's stage cases.  small: the host test's versions, framing
    reduced to what a block of 105 * 2^3 bytes carries (D = 8 for the decimator; the conditioning cases have blocks of their
    own, see small_cond_record)."""
    out = {
        "filter_record": (Notch(255 if not small else 31, 14), rec),
        "iq_to_if": (IQ(63 if not small else 15, 14), rec),
        "requantize_int16": (Requant(np.int16, 40, 13), rec),
        "requantize_float32": (Requant(np.float32, scale=2.0 ** -20), rec),
        "resample_16_1": (Resamp(16, 1, 129 if not small else 33), rec.head((rec.B >> 4) + (16384 if not small else 48))),
        "resample_4_3": (Resamp(4, 3, 97 if not small else 17), rec),
        "decimate": (Decim(16 if not small else 8, 31), rec),
    }
    if not small:
        out["condition_int8"] = (Cond(rec, np.int8, 1, 8192), rec)
        out["condition_int16"] = (Cond(rec, np.int16, 2, 2048), rec)
    return out


def small_cond_cases():
    """The conditioning cases at B = 2^20 with a block of 105 * 2^10 bytes: the smallest blocks the stage takes (256 frames)
    tile it."""
    rec = Tiled(1 << 20, 105 << 10, extra=48 * 5)
    return {"condition_int8": (Cond(rec, np.int8, 1, 256), rec), "condition_int16": (Cond(rec, np.int16, 2, 256), rec)}


# ---- the strong-signal cancellation ----------------------------------------------------------------------------------------

class CancelPlan(object):
    """Four hand-made channels (cancel_cases.handmade: blocks of 2046 samples at 2.046 Msps) on a tiled record of n = B + extra
    bytes, B a multiple of the kernel's tile of 4096:
      A  5 blocks that straddle B / 2
      B  6 blocks that straddle B, block 2 starting exactly at B: a tile's first sample at a 33-bit position
      C  4 blocks of which the last ends with the record's last sample
      D  5 blocks that start in the first tile
    with amplitudes of some tens of LSB on full-scale bytes, so that the bytes change and some clip.  A channel's window is
    its blocks with MARGIN samples (more than a tile) either side, cut at the record's ends; the windows are disjoint, so the
    record's clip count is the sum of theirs.  Two further windows that no block touches lie across B / 2 + Q and B - Q,
    Q = min(2^20, B / 8): there the output is the input.  expect() is cancel_spec.cancel on the window's bytes with the
    channel rebased to the window's first byte."""
    MARGIN = 5000
    BLOCKS = dict(A=5, B=6, C=4, D=5)

    def __init__(self, rec, seed=0xCA9C):
        self.rec = rec
        B, n = rec.B, rec.n
        assert B % 4096 == 0
        rng = np.random.default_rng(seed)
        self.s = orc.OracleSettings(samplingFreq=cancel_cases.LOW_FS, IF=cancel_cases.LOW_IF, numberOfChannels=4, msToProcess=6.0)
        ms = 6
        self.names, self.chans, rows, self.ms_done, self.windows = [], [], [], [], []
        for i, name in enumerate("ABCD"):
            done = self.BLOCKS[name]
            prn, freq = 4 + 7 * i, cancel_cases.LOW_IF + float(rng.integers(-4000, 4001))
            code = cancel_cases.CHIP_RATE + rng.uniform(-3.0, 3.0, ms)
            carr = freq + rng.uniform(-20.0, 20.0, ms)
            ends = cancel_cases.handmade(self.s, 0, freq, code, carr)[0].astype(np.int64)    # block ends of a channel from 0
            start = {"A": B // 2 - int(ends[1]) - 777, "B": B - int(ends[1]), "C": n - int(ends[done - 1]), "D": 100}[name]
            series = cancel_cases.handmade(self.s, start, freq, code, carr)
            assert np.array_equal(series[0], ends + start)
            self.names.append(name)
            self.chans.append((prn, freq, float(start)))
            rows.append(series)
            self.ms_done.append(done)
            self.windows.append((max(0, start - self.MARGIN), min(n, start + int(ends[done - 1]) + self.MARGIN)))
        self.series = np.stack(rows)
        self.ms_done = np.array(self.ms_done, dtype=np.int32)
        self.amp = rng.uniform(-45.0, 45.0, (4, ms, 2))
        q = min(1 << 20, B // 8)
        self.quiet = [(B // 2 + q - 4096 - 3, B // 2 + q + 4096 + 5), (B - q - 4096 - 3, B - q + 4096 + 5)]
        a, b, c, d = (dict(zip(self.names, self.chans))[k][2] for k in "ABCD")
        end = lambda k: int(self.series[self.names.index(k), 0, self.BLOCKS[k] - 1])
        assert a < B // 2 < end("A") and b < B < end("B") and B in self.series[1, 0, :].astype(np.int64) and end("C") == n
        assert d < 4096
        spans = sorted(self.windows + self.quiet)
        assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:])) and spans[0][0] == 0 and spans[-1][1] == n, spans

    def expect(self, at, i, w0, w1):
        """(y, v, clipped, covered) of the contract on window i: bytes [w0, w1) through `at`, channel i alone, rebased."""
        prn, freq, start = self.chans[i]
        series = np.array(self.series[i:i + 1])
        series[:, 0] -= w0
        return cancel_spec.cancel(self.s, at(w0, w1), 0, [(prn, freq, start - w0)], series, self.ms_done[i:i + 1],
                                  self.amp[i:i + 1])

    def contract(self, i):
        return lambda at, w0, w1: self.expect(at, i, w0, w1)[0]


# ---- the monitor --------------------------------------------------------------------------------------------------------

def waterfall_whole(rec, N, tail, fs_mhz):
    """What sgx_probe_waterfall must give on the tiled record at offset 0, n = B + N + tail, noverlap = 0, S = B: one full
    slice of B / N segments and one kept slice of one segment.  The integers come from the block by multiplication
    (Tiled.sums); slice 0's spectrum is the mean over its segments, which start at only P / gcd(P, N) different phases of the
    period: each phase's spectrum once, weighted by how often it occurs."""
    B, n = rec.B, rec.B + N + tail
    assert tail < N and n <= rec.n and B % N == 0
    plan = waterfall_spec.plan(n, N, 0, B)
    assert plan == [(0, B, B // N), (B, N + tail, 1)]
    w = waterfall_spec.window(N)
    scale = 1.0 / (fs_mhz * float((w * w).sum()))
    two = np.ones(N // 2 + 1)
    two[1:-1] = 2.0
    phases, counts = np.unique((np.arange(B // N, dtype=np.int64) * N) % rec.P, return_counts=True)
    acc = np.zeros(N // 2 + 1)
    for p, c in zip(phases, counts):
        acc += float(c) * ((waterfall_spec.segment_spectrum(rec.at(p, p + N), w) * scale) * two)
    pxx = np.stack([acc / float(B // N), (waterfall_spec.segment_spectrum(rec.at(B, B + N), w) * scale) * two])
    moments, hist = np.zeros((2, 4), dtype=np.int64), np.zeros((2, 256), dtype=np.int64)
    for j, (a, b) in enumerate(((0, B), (B, n))):
        m, hist[j] = rec.sums(a, b)
        moments[j] = m
    return dict(pxx=pxx, moments=moments, hist=hist, n_segments=np.array([B // N, 1], dtype=np.int64), phases=phases.size)


# ---- the windows of the GPU test, so that the host test can hold every one of them to the rule ------------------------------

SPC = 38192                           # samples per code period of the default front end
SCENE_N = B32 + 100 * SPC             # scene8: the default scene, made on the device
SYNTH_WINDOWS = ((B32 // 2 - 5000, B32 // 2 + 5000), (B32 - 5000, B32 + 5000), (SCENE_N - 10000, SCENE_N))
SYNTH_CALL = (B32 + 7 * SPC + 3, 20011)                                       # (offset, n) of one call with offset > 2^32
PROBE_WINDOWS = ((B32 + 12345, B32 + 12345 + 10 * SPC), (B32 - 5 * SPC - 3, B32 + 5 * SPC - 3))
ACQ_WINDOW = (B32 - SPC - 7, B32 + 11 * SPC - 7)                              # 11 periods, 12 for the coherent search
TRACK_BEFORE, TRACK_MS = 20, 80       # the run starts 20 code periods before the boundary and goes 60 ms past it
TRACK_START = B32 - TRACK_BEFORE * SPC
TRACK_WINDOW = (TRACK_START, TRACK_START + (TRACK_MS + 13) * SPC)              # the acquisition's 11 periods, then 80 blocks
WF_SEGMENT, WF_TAIL = 16384, 1000
WF_SECOND = (B32 - 3, 3 * 16384, 16384)                                       # (offset, n, N = S) of the second monitor call
FILE_WINDOWS = ((4096 + 5, 4096 + 5 + 6000), (B32 // 2 - 3000, B32 // 2 + 3000), (B32 - 3000, B32 + 3000))
FILE_TAIL = 70001
LOW_FS, LOW_IF, LOW_SPC = 4092000.0, 1023000.0, 4092                          # the low-rate front end of two tracking cases
LOW_SCENE = (0xB16 + 4092, LOW_FS, LOW_IF, [2, 5], [1750.0, -3300.0], [4092 // 3, 4092 - 5], [9, 8])     # Scene.make's arguments
LOW_N = B32 + 100 * LOW_SPC
PROBE_RULE = 40000                    # the rule is held on this many bytes of a scene window: a prefix that differs will do


def scene_reader(generate, scene):
    """at() of a scene record: the generator is a pure function of the position; in front of the record there is nothing."""
    def at(a, b):
        a, b = int(a), int(b)
        out = np.zeros(b - a, dtype=np.int8)
        if b > 0:
            out[max(0, -a):] = generate(scene, b - max(a, 0), offset=max(a, 0))
        return out
    return at


def sparse_reader(n, start, payload, fill=0):
    """at() of a sparse record of n bytes: `fill` everywhere but `payload` (any array, its bytes) from byte `start` on; the
    filler goes on outside the record."""
    raw = np.ascontiguousarray(payload).view(np.uint8).ravel()
    assert 0 <= start and start + raw.size <= n

    def at(a, b):
        pos = np.arange(int(a), int(b), dtype=np.int64)
        out = np.full(pos.size, fill, dtype=np.uint8)
        inside = (pos >= start) & (pos < start + raw.size)
        out[inside] = raw[pos[inside] - start]
        return out.view(np.int8)
    return at


def typed_start(itemsize, spc=SPC):
    """The byte at which the payload of a sparse record of this sample width starts: 20 code periods before byte 2^32."""
    return B32 - TRACK_BEFORE * spc * itemsize


def low_rate_window():
    return typed_start(1, LOW_SPC), typed_start(1, LOW_SPC) + (TRACK_MS + 13) * LOW_SPC


# The coherent run on the low-rate window (sgx_track_coherent; tests/coh_track_spec.py): groups of 4 blocks behind a pull-in of
# 40, given edges.  A channel starts within the acquisition's 11 periods of the window's start, TRACK_BEFORE periods before
# byte 2^32: the boundary falls in the pull-in, and every group (k0 = 43, 51) reads at 33-bit positions.
LOW_COHERENT = dict(T=4, P=40, H=100, edges=(3, 11))


def low_rate_coherent_window():
    """The bytes the coherent phase of that run reads at the least: from the latest start of its first group (a channel that
    begins 11 periods into the window, blocks of at most LOW_SPC + 1 samples) to the end of a channel's 80 blocks that
    begins at the window's start (blocks of at least LOW_SPC - 1)."""
    w0, _ = low_rate_window()
    k0 = max(LOW_COHERENT["P"] + (e - LOW_COHERENT["P"]) % 20 for e in LOW_COHERENT["edges"])
    return w0 + 11 * LOW_SPC + k0 * (LOW_SPC + 1), w0 + TRACK_MS * (LOW_SPC - 1)


def scene_windows():
    """Every window of scene8 that the GPU test reads, by the name of what reads it."""
    out = dict(("synth-%d" % i, w) for i, w in enumerate(SYNTH_WINDOWS))
    out["synth-call"] = (SYNTH_CALL[0], SYNTH_CALL[0] + SYNTH_CALL[1])
    out.update(("probe-%d" % i, w) for i, w in enumerate(PROBE_WINDOWS))
    out["acquire"] = ACQ_WINDOW
    out["track"] = TRACK_WINDOW
    return out


def first_code_start(sat, at_least):
    """The first sample >= at_least at which this satellite of a scene (synth.Scene.sats entry) starts a code period: exact,
    from the generator's own 32.32 code NCO."""
    period = 1023 << 32
    phase = (int(at_least) * sat["code_fcw"] + sat["code_c0"]) % period
    if phase < sat["code_fcw"]:
        return int(at_least)
    return int(at_least) + -(-(period - phase) // sat["code_fcw"])
