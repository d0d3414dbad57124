"""Records that go silent - stretches of samples that are exactly zero - and what the reference does with them.  Test
infrastructure only (tests/test_silent_host.py holds every expectation here against the oracle alone, tests/test_silent_gpu.py
runs the product on the same arrays); needs no GPU.

Exact zeros are the one input on which the reference's arithmetic leaves the finite numbers.  In the search peak / second
peak is 0 / 0.  In tracking the first block whose six sums are exactly zero makes both discriminators NaN (arctan(0 / 0),
(0 - 0) / (0 + 0)), the NCOs, codeFreq and carrFreq follow, and at the next block the reference dies in int(np.ceil(nan))
with "ValueError: cannot convert float NaN to integer" (tracking.py:148-151).

SEARCH: name -> the array a search is handed (11 ms of the default front end unless said otherwise).
TRACKING: name -> where the 41 ms default scene is silenced, in ms relative to the first sample of channel 0's block 12.
FAMILIES: one launch per tracking kernel family - the front end, the sample type, the channels and the environment that select
it - and the kernel sgx_timing.track_kernel must then report.
"""
import functools

import numpy as np

from conftest import pkg
from oracle import softgnss_oracle as orc

N = 38192                      # samples per code of the default front end (38.192 Msps, IF 9.548 MHz)
SEARCH_MS, TRACK_MS = 11, 30   # the search reads 11 ms (the fine search: codePhase + 10 ms); tracking cases track 30 ms
RECORD_MS = SEARCH_MS + TRACK_MS
GAP_BLOCK = 12                 # the silence starts in the middle of channel 0's block 12
NOISE_SEED, NOISE_SIGMA = 20261021, 24.0
NONFINITE_AT = N + 12345       # in the SECOND search block: "the later block wins unless the earlier maximum is larger"
#                                (acquisition.py:129-133) then keeps the block whose every power is NaN
TIE_GAP = 1e-6                 # coherent_acq_spec.rel_gap below this: an arg-max too close to a tie to compare
COHERENT_PRNS = (0, 2, 6, 10, 1, 4)   # PRN indices the 2 x 2 ms searches look at: PRN 1, 3, 7, 11 of the scene, 2 and 5 absent


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scene(fs=38192000.0, IF=9548000.0, ms=RECORD_MS):
    """int8 record: the default scene at the default front end; two satellites (PRN 2, 5) at any other, as
    test_other_front_ends_against_oracle places them."""
    synth = pkg("synth")
    n = int(round(fs / 1000))
    if fs == 38192000.0:
        sc = synth.Scene.default()
    else:
        sc = synth.Scene.make(0xFE000 + n, fs, IF, [2, 5], [1750.0, -3300.0], [n // 3, n - 5], [9, 8])
    return _frozen(synth.generate(sc, ms * n))


# ---- search ------------------------------------------------------------------------------------------------------------------
def _zeroed(lo, hi):
    x = scene()[:SEARCH_MS * N].copy()
    x[lo:hi] = 0
    return x


def _nonfinite(value):
    x = scene()[:SEARCH_MS * N].astype(np.float64)
    x[NONFINITE_AT] = value
    return x


@functools.lru_cache(maxsize=None)
def noise_record():
    """RECORD_MS of Gaussian int8 noise; the search case is its first SEARCH_MS."""
    rng = np.random.default_rng(NOISE_SEED)
    return _frozen(np.clip(np.rint(rng.normal(0.0, NOISE_SIGMA, RECORD_MS * N)), -127, 127).astype(np.int8))


SEARCH = {
    "scene": lambda: scene()[:SEARCH_MS * N].copy(),                        # the untouched default scene, for comparison
    "zeros-int8": lambda: np.zeros(SEARCH_MS * N, dtype=np.int8),
    "zeros-float64": lambda: np.zeros(SEARCH_MS * N, dtype=np.float64),
    "zeros-uint8": lambda: np.zeros(SEARCH_MS * N, dtype=np.uint8),         # bytes of value 0 (128 would be a constant, not silence)
    "noise-only": lambda: noise_record()[:SEARCH_MS * N].copy(),            # Gaussian int8 noise: nothing to detect
    "first-ms-silent": lambda: _zeroed(0, N),                               # the block choice is decisive: block 1 ...
    "second-ms-silent": lambda: _zeroed(N, 2 * N),                          # ... respectively block 0, for every PRN
    "late-signal": lambda: np.zeros(SEARCH_MS * N, dtype=np.int8),          # (the record: late_signal_record())
    "nan-sample": lambda: _nonfinite(np.nan),
    "inf-sample": lambda: _nonfinite(np.inf),
}
ALL_NAN = ("zeros-int8", "zeros-float64", "zeros-uint8", "late-signal", "nan-sample", "inf-sample")   # NaN metrics, freqBin 0
BLOCK_SEL = {"first-ms-silent": 1, "second-ms-silent": 0}


@functools.lru_cache(maxsize=None)
def search_signal(name):
    return _frozen(SEARCH[name]())


def late_signal_record():
    """11 ms of zeros, then the default scene: nothing is found, the tracking that follows has no channel."""
    return np.concatenate([np.zeros(SEARCH_MS * N, dtype=np.int8), scene()])


def oracle_settings(fs=38192000.0, IF=9548000.0, **kw):
    return orc.OracleSettings(samplingFreq=fs, IF=IF, **kw)


@functools.lru_cache(maxsize=None)
def search_expect(name, path="acquire"):
    """The reference's outputs for search case `name` on one of the product's paths:
    acquire / noncoh - oracle.acquire on the array itself (2 blocks; noncoh: their sum);
    f64 - what sgx_acquire_f64 is handed, the array as float64: the same values in the same float64 arithmetic (the oracle
    promotes every sample type in its first product), so the same expectation;
    coherent / coherent-noncoh - tests/coherent_acq_spec.py, 2 windows of 2 ms, the PRN indices COHERENT_PRNS."""
    if path == "f64":
        return search_expect(name, "acquire")
    x = search_signal(name)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if path in ("coherent", "coherent-noncoh"):
            import coherent_acq_spec as spec
            return spec.acquire(oracle_settings(), x, 2, 2, path == "coherent-noncoh", None, prn_indices=list(COHERENT_PRNS),
                                details=True)
        return orc.acquire(oracle_settings(), x, noncoh=(path == "noncoh"))


ANY_RATE = (16367600.0, 4130400.0)   # N = 16 368 is not the four-step length: the any-rate search on a padded transform
ANY_N = 16368
ANY_RATE_CASES = tuple(SEARCH)       # every search case again, built for this rate


@functools.lru_cache(maxsize=None)
def any_rate_signal(name):
    """Search case `name` for the any-rate front end: the same construction on SEARCH_MS of that rate's two-satellite scene
    (scene(*ANY_RATE)), with ANY_N samples per code - the silent code period and the sample that is not finite lie where they
    lie at the default rate, counted in code periods."""
    n = SEARCH_MS * ANY_N
    base = scene(*ANY_RATE)[:n]
    if name == "scene":
        x = base.copy()
    elif name in ("zeros-int8", "zeros-float64", "zeros-uint8", "late-signal"):
        x = np.zeros(n, dtype=search_signal(name).dtype)
    elif name == "noise-only":
        x = noise_record()[:n].copy()
    elif name in BLOCK_SEL:
        x = base.copy()
        b = 1 - BLOCK_SEL[name]                       # the silent block: the other one is chosen
        x[b * ANY_N:(b + 1) * ANY_N] = 0
    else:
        x = base.astype(np.float64)
        x[ANY_N + 123] = {"nan-sample": np.nan, "inf-sample": np.inf}[name]
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def any_rate_expect(name, noncoh=False):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return orc.acquire(oracle_settings(*ANY_RATE), any_rate_signal(name), noncoh=noncoh)


def clear_of_a_tie(x, noncoh=False, fs=38192000.0, IF=9548000.0):
    """bool[32]: the oracle's arg-maxes over the bins of the search of `x` - the one that decides freqBin - lie at least
    TIE_GAP (relative) clear of the runner-up: the rule of coherent_acq_spec.rel_gap."""
    import coherent_acq_spec as spec
    s = oracle_settings(fs, IF)
    g = spec.grid(s, 1, 2, noncoh, 500.0)
    sp = np.fft.fft(spec.fold(s, np.asarray(x, dtype=np.float64), g), axis=-1)
    table = orc.make_ca_table(s)
    out = np.zeros(32, dtype=bool)
    for p in range(32):
        res, _ = spec.coarse(s, sp, g, np.fft.fft(table[p]).conj())
        out[p] = spec.rel_gap(spec._top2(res.max(1))) >= TIE_GAP
    return out


# ---- tracking ----------------------------------------------------------------------------------------------------------------
# (start, length) of the silence in ms, counted from the first sample of channel 0's block GAP_BLOCK; None: to the record's end.
# "start" -inf: from the first tracked sample (the smallest codePhase) on.
TRACKING = {
    "silent-from-k": (0.5, None),       # block 12 partly silent and finite, block 13 the first with zero sums
    "silent-from-start": (-np.inf, None),   # block 0 is NaN
    "one-block-gap": (0.5, 1.5),        # signal again after 1.5 ms: the NaN state is sticky, the reference still dies
    "short-gap": (0.5, 0.4),            # no block entirely silent: nothing is NaN, the run completes
}
MUST_RAISE = ("silent-from-k", "silent-from-start", "one-block-gap")


class Family(object):
    """One tracking launch: front end (fs, IF), numpy sample type, how the int8 scene becomes that type (`convert`), the
    channels (`repeat` copies of the acquired ones), the environment and the kernel it must select."""

    def __init__(self, name, kernel, dtype="int8", fs=38192000.0, IF=9548000.0, convert=None, repeat=1, env=None, nch=8,
                 members=None, chained=False, data=None):
        self.name, self.kernel, self.dtype, self.fs, self.IF = name, kernel, np.dtype(dtype), fs, IF
        self.data = data or name          # the family whose record and expectation this one shares
        self.convert = convert or (lambda x: x)
        self.repeat, self.env, self.nch, self.members, self.chained = repeat, dict(env or {}), nch, members, chained


LOW, LOW_IF = 4092000.0, 1023000.0        # trk_kernel_multi: four samples per chip
ANY, ANY_IF = 5456000.0, 1364000.0        # trk_kernel_any: int16 below 16 samples per chip
FAMILIES = [
    Family("trk3", 5),
    Family("trk2", 2, env={"SGX_TRK_V3": "0"}, members=30, data="trk3"),
    Family("trk2-one-workgroup", 2, env={"SGX_TRK_SPLIT": "1"}, members=1, data="trk3"),
    Family("tp", 3, repeat=17, members=1, data="trk3"),                                 # 136 channels: the 8 replicated
    Family("multi", 4, fs=LOW, IF=LOW_IF, nch=2),
    Family("int16", 2, dtype="<i2", convert=lambda x: x.astype("<i2") * 129),
    # uint8: offset-binary bytes tracked as they are, so the silent stretch is byte 0 - a constant 128 is not silent
    Family("uint8", 5, dtype="u1", convert=lambda x: (x.astype(np.int16) + 128).astype(np.uint8)),
    Family("float32-narrowed", 5, dtype="<f4", convert=lambda x: x.astype("<f4") / 32.0),        # integers x 2^-5: exact
    Family("float64-scaled", 2, dtype="<f8", convert=lambda x: x.astype("<f8") * 1.234567890123e-3),
    Family("per-sample", 6, dtype="<i2", fs=ANY, IF=ANY_IF, nch=2, convert=lambda x: x.astype("<i2") * 129),
    Family("queued", 5, chained=True, data="trk3"),
]
FAMILY = {f.name: f for f in FAMILIES}


@functools.lru_cache(maxsize=None)
def channels(fs=38192000.0, IF=9548000.0, nch=8):
    """The oracle's search and preRun of the untouched record: dict PRN / acquiredFreq / codePhase / status."""
    s = oracle_settings(fs, IF, numberOfChannels=nch)
    if fs != 38192000.0:
        s.acqSatelliteList = range(1, 7)
    n = s.samplesPerCode
    return orc.pre_run(s, orc.acquire(s, scene(fs, IF)[:SEARCH_MS * n]))


def track_settings(fam, ms=TRACK_MS):
    return oracle_settings(fam.fs, fam.IF, numberOfChannels=fam.nch, msToProcess=float(ms), dataType=fam.dtype.str)


def start_bytes(fam):
    """codePhase of every channel for this family's sample type: the reference seeks BYTES (tracking.py:107), so the
    channel that starts at sample c of the int8 record starts at byte c x itemsize."""
    ch = channels(fam.fs, fam.IF, fam.nch)
    return np.asarray(ch["codePhase"], dtype=np.int64) * fam.dtype.itemsize


@functools.lru_cache(maxsize=None)
def _gap_origin(fs, IF, nch):
    """Sample index of the first sample of channel 0's block GAP_BLOCK on the untouched int8 record."""
    fam = Family("origin", 0, fs=fs, IF=IF, nch=nch)
    ch = channels(fs, IF, nch)
    st = orc.TrackStepper(track_settings(fam), ch["PRN"][0], ch["acquiredFreq"][0], ch["codePhase"][0], scene(fs, IF))
    for _ in range(GAP_BLOCK):
        st.step()
    return st.pos


def silent_span(case, fam):
    """[lo, hi) in samples of the stretch case `case` silences in this family's record."""
    start, length = TRACKING[case]
    n = int(round(fam.fs / 1000))
    total = RECORD_MS * n
    if start == -np.inf:
        lo = int(np.min(channels(fam.fs, fam.IF, fam.nch)["codePhase"]))
    else:
        lo = _gap_origin(fam.fs, fam.IF, fam.nch) + int(round(start * n))
    hi = total if length is None else lo + int(round(length * n))
    return lo, hi


@functools.lru_cache(maxsize=None)
def track_record(case, family):
    """The family's record (its sample type) with the case's stretch set to zero: bytes of value 0 whatever the type."""
    fam = FAMILY[family]
    if fam.data != family:
        return track_record(case, fam.data)
    x = np.ascontiguousarray(fam.convert(scene(fam.fs, fam.IF)), dtype=fam.dtype).copy()
    lo, hi = silent_span(case, fam)
    x[lo:hi] = 0
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def track_expect(case, family):
    """Per channel of the family (before replication): dict k - the index of the first block whose six sums are exactly zero,
    None if there is none within TRACK_MS; rows - float64[13, blocks run]: the values TrackStepper.step() returned, up to and
    including block k; raises - step() of block k + 1 raised ValueError (k None: False, all TRACK_MS blocks ran)."""
    fam = FAMILY[family]
    if fam.data != family:
        return track_expect(case, fam.data)
    s = track_settings(fam)
    ch = channels(fam.fs, fam.IF, fam.nch)
    rec = track_record(case, family)
    phase = start_bytes(fam)
    out = []
    for c in range(len(ch["PRN"])):
        if ch["PRN"][c] == 0:
            continue
        st = orc.TrackStepper(s, ch["PRN"][c], ch["acquiredFreq"][c], float(phase[c]), rec)
        rows, k, raised = [], None, False
        for it in range(TRACK_MS):
            try:
                with np.errstate(divide="ignore", invalid="ignore"):
                    row = st.step()
            except ValueError as e:
                assert "NaN" in str(e), e
                raised = True
                break
            assert row is not None, "the record is long enough for every case"
            rows.append(row)
            if k is None and all(v == 0.0 for v in row[3:9]):
                k = it
        out.append(dict(k=k, rows=np.array(rows, dtype=np.float64).T, raises=raised))
    return out


def first_silent(case, family):
    """(channel, k) of the lowest-numbered channel that goes silent, or None."""
    for c, e in enumerate(track_expect(case, family)):
        if e["k"] is not None:
            return c, e["k"]
    return None
