"""Tracking at full-scale samples on every kernel and record path, against the numpy oracle.

Every typed tracking kernel sums in fixed point (sgx_trk3.hip: 48-bit payloads at 2^30; sgx_trk2.hip: 2^28, int16 2^24 /
2^19; sgx_trk_tp.hip: int32 digit sums; sgx_trk_multi / sgx_trk_any: their own).  The synthetic scene never gets near
those limits; the records of tests/full_scale.py do (noiseless ones that line up with the replica, 1-bit ones, the
default scene overdriven into the rails).  Each case: absoluteSample bit-exact, the six correlator series within TRK_TOL,
the kernel the plan (sgx_trk.hip: trk_plan) names is the one that ran - or, for the speculative kernel (5), the round-3
kernel (2) exactly when the record is too strong for it, said on stderr."""
import os

import numpy as np
import pytest

from conftest import pkg
from oracle import softgnss_oracle as orc
import full_scale as fsr
from test_gpu_parity import TRK_TOL, _trk_err

pytestmark = pytest.mark.gpu

MS = 50
TOO_STRONG = "too strong for the speculative kernel"
SCAN_LINE = "the round-3 kernel tracks this record"          # (the host scan's; a repeated launch says "repeating ...")
ABOVE = ["clean%d" % a for a in fsr.INT8_ABOVE]
# the big file for the streaming entry paths: its first stretch repeated (a record still loading when tracking starts)
BIG_FILE_BYTES = 128 << 20


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _settings(m, dtype="int8", nch=1, ms=MS, front=None):
    s = m.Settings()
    so = orc.OracleSettings()
    for o in (s, so):
        if front is not None:
            o.samplingFreq, o.IF = front
        o.dataType, o.numberOfChannels, o.msToProcess, o.skipNumberOfBytes = dtype, nch, float(ms), 0
    return s, so


def _chans(base, isz):
    """(PRN, freq, first sample) -> the C-ABI's (PRN, freq, codePhase in BYTES) and the oracle's channel table."""
    chans = [(int(p), float(f), float(st * isz)) for p, f, st in base]
    table = dict(PRN=np.array([c[0] for c in chans]), acquiredFreq=np.array([c[1] for c in chans]),
                 codePhase=np.array([c[2] for c in chans]), status=['T'] * len(chans))
    return chans, table


def _oracle(so, table, raw, ms=MS):
    so.numberOfChannels, so.msToProcess = len(table["PRN"]), float(ms)
    return orc.stack_series(orc.track(so, table, raw))


def _check(got, done, want, ms=MS, tag=None):
    assert np.all(done == ms), (tag, done)
    assert np.array_equal(got[:, 0], want[:, 0]), tag                    # absoluteSample bit-exact
    err = _trk_err(got, want)
    assert err < TRK_TOL, (tag, err)


def _ran(ctx, capfd, want_kernel, tag, members=None):
    """The kernel that ran is want_kernel (and the members); -> (timing, what the call printed on stderr)."""
    tm = ctx.timing()
    err = capfd.readouterr().err
    assert tm["track_kernel"] == want_kernel, (tag, tm, err)
    if members is not None:
        assert tm["track_members"] == members, (tag, tm)
    return tm, err


def _run(ctx, rec, chans, ms, code, env=None):
    return _with_env(env or {}, lambda: ctx.track(rec, chans, ms, data_type=code))


# ---- sample types x kernels (resident records) ----------------------------------------------------------------------

def _v3_expect(name, dtype):
    """Whether the speculative kernel keeps a record of tests/full_scale.py at the default front end.
    int8: magnitudes below the bound (test_full_scale_records.py) AND unit prompt sums below half the payload's room
    (2^16: the kernel's own look at them, round 5) - amplitude 50 (51 200 per unit); amplitude 80 has 81 900.
    uint8 (no magnitude bound: the DC of 128): the prompt look only - a 1-bit or amplitude-127 record is past 2^16,
    the overdriven scene (noise at the rails, prompt sums of a few 10^4) is not."""
    if dtype == "int8":
        return name == "clean50"
    return name == "saturated"


def _default_records(m, s, dtype, ms=MS):
    """name -> (record, channel base) at the default front end."""
    out = {}
    if dtype == "int8":
        for name, (x, _) in fsr.int8_records(m, s, ms).items():
            out[name] = x
    else:
        top = 127 if dtype == "uint8" else 32000
        out["clean%d" % top] = fsr.as_type(fsr.clean_record(m, s, top, ms), dtype)
        out["clipped"] = fsr.clipped_record(m, s, dtype, ms)
        out["saturated"] = fsr.saturated_record(m, s, dtype, ms)
    return {k: (v, fsr.saturated_channels(s) if k == "saturated" else [fsr.clean_channel(s)]) for k, v in out.items()}


@pytest.mark.parametrize("dtype", ["int8", "uint8"])
def test_speculative_kernel_and_round3_kernel_layouts_at_full_scale(dtype, capfd):
    """Kernel 5 at the default front end (or kernel 2 when the record is too strong for it, said on stderr); kernel 2
    with SGX_TRK_V3=0 (three members per unit and arm: 30) and SGX_TRK_SPLIT=1 (one member owns all ten units: the
    layout whose scale drops by the unit count); kernel 3 with 130 replicated channels (row 0 against the oracle, every
    replica identical)."""
    m = pkg()
    s, so = _settings(m, dtype)
    code = {"int8": m._native.DT_INT8, "uint8": m._native.DT_UINT8}[dtype]
    ctx = m.engine.get_context(s, 0)
    for name, (raw, base) in _default_records(m, s, dtype).items():
        chans, table = _chans(base, 1)
        want = _oracle(so, table, raw)
        rec = ctx.upload_bytes(raw)
        try:
            capfd.readouterr()
            got, done = _run(ctx, rec, chans, MS, code)
            keep = _v3_expect(name, dtype)
            _, err = _ran(ctx, capfd, 5 if keep else 2, (dtype, name), 20 if keep else None)
            assert (TOO_STRONG in err) == (not keep), (dtype, name)
            _check(got, done, want, tag=(dtype, name))
            for env, members in (({"SGX_TRK_V3": "0"}, 30), ({"SGX_TRK_SPLIT": "1"}, 1)):
                got, done = _run(ctx, rec, chans, MS, code, env)
                _, err = _ran(ctx, capfd, 2, (dtype, name, env), members)
                assert TOO_STRONG not in err
                _check(got, done, want, tag=(dtype, name, env))
            many, dm = _run(ctx, rec, [chans[i % len(chans)] for i in range(130)], MS, code)
            _, err = _ran(ctx, capfd, 3, (dtype, name, "tp"), 1)
            assert TOO_STRONG not in err
            _check(many[:len(chans)], dm[:len(chans)], want, tag=(dtype, name, "tp"))
            assert all(np.array_equal(many[i], many[i % len(chans)]) for i in range(len(chans), 130)), (dtype, name)
        finally:
            rec.free()


def test_int16_at_full_scale_every_layout():
    """int16 records at full scale (a noiseless amplitude of 32 000, 1-bit at +-32 767, the overdriven scene): kernel 2
    in its default layout (30 members) and with one member owning all ten units (SGX_TRK_SPLIT=1: 2^24 in the lanes,
    2^19 in the granules, less per unit), kernel 3 with 130 replicas."""
    m = pkg()
    s, so = _settings(m, "int16")
    code = m._native.DT_INT16
    ctx = m.engine.get_context(s, 0)
    for name, (raw, base) in _default_records(m, s, "int16").items():
        chans, table = _chans(base, 2)
        want = _oracle(so, table, raw)
        rec = ctx.upload_bytes(raw)
        try:
            for env, members in (({}, 30), ({"SGX_TRK_SPLIT": "1"}, 1)):
                got, done = _run(ctx, rec, chans, MS, code, env)
                tm = ctx.timing()
                assert tm["track_kernel"] == 2 and tm["track_members"] == members, (name, env, tm)
                _check(got, done, want, tag=(name, env))
            many, dm = _run(ctx, rec, [chans[i % len(chans)] for i in range(130)], MS, code)
            assert ctx.timing()["track_kernel"] == 3, name
            _check(many[:len(chans)], dm[:len(chans)], want, tag=(name, "tp"))
            assert all(np.array_equal(many[i], many[i % len(chans)]) for i in range(len(chans), 130)), name
        finally:
            rec.free()


def test_low_rate_front_end_at_full_scale():
    """5.456 MHz (5.3 samples per chip): int8 on kernel 4, uint8 and int16 on kernel 6 - noiseless full-scale, 1-bit and
    overdriven records."""
    m = pkg()
    ms = 40
    for dtype, kernel in (("int8", 4), ("uint8", 6), ("int16", 6)):
        s, so = _settings(m, dtype, ms=ms, front=fsr.LOW_RATE)
        code = {"int8": m._native.DT_INT8, "uint8": m._native.DT_UINT8, "int16": m._native.DT_INT16}[dtype]
        isz = np.dtype(dtype).itemsize
        ctx = m.engine.get_context(s, 0)
        top = 32000 if dtype == "int16" else 127
        ch = [fsr.clean_channel(s, start=3000)]
        recs = {"clean": (fsr.as_type(fsr.clean_record(m, s, top, ms, start=3000), dtype), ch),
                "clipped": (fsr.clipped_record(m, s, dtype, ms, start=3000), ch),
                "saturated": (fsr.saturated_record(m, s, dtype, ms),
                              [(1, s.IF + 1250.0, 12345 % s.samplesPerCode), (14, s.IF + 2900.0, 777)])}
        for name, (raw, base) in recs.items():
            chans, table = _chans(base, isz)
            want = _oracle(so, table, raw, ms)
            rec = ctx.upload_bytes(raw)
            try:
                got, done = _run(ctx, rec, chans, ms, code)
                assert ctx.timing()["track_kernel"] == kernel, (dtype, name, ctx.timing())
                _check(got, done, want, ms, tag=(dtype, name))
            finally:
                rec.free()


def test_float_records_at_full_scale():
    """float32 / float64 versions of the noiseless amplitude-127 record times 2^20 (float32, integers times a power of two:
    narrowed to int8 exactly, then too strong for kernel 5 - kernel 2, the series scaled back by 2^20); the same before
    its rounding (the latency-mode kernel's float instance, scaled by 2^-20 on conversion: kernel 2, 10 members); and
    float32 with one outlier 2^12 times the mean |x| (out of range: the per-sample kernel 6)."""
    m = pkg()
    for dtype, code_name in (("float32", "DT_FLOAT32"), ("float64", "DT_FLOAT64")):
        s, so = _settings(m, dtype)
        code = getattr(m._native, code_name)
        isz = np.dtype(dtype).itemsize
        ctx = m.engine.get_context(s, 0)
        chans, table = _chans([fsr.clean_channel(s)], isz)
        # (float64 is never narrowed: the latency-mode kernel's float instance takes both)
        cases = [("integers", fsr.float_record(fsr.clean_record(m, s, 127, MS), dtype), 2,
                  None if dtype == "float32" else 10),
                 ("scaled", fsr.float_record(fsr.unrounded_record(m, s, 127, MS), dtype), 2, 10)]
        if dtype == "float32":
            out = fsr.float_record(fsr.unrounded_record(m, s, 127, MS), dtype)
            out[20 * s.samplesPerCode + 77] = np.float32(2.0 ** 20 * 127 * 8192)
            cases.append(("outlier", out, 6, None))
        for name, raw, kernel, members in cases:
            want = _oracle(so, table, raw)
            rec = ctx.upload_bytes(raw)
            try:
                got, done = _run(ctx, rec, chans, MS, code)
                tm = ctx.timing()
                assert tm["track_kernel"] == kernel, (dtype, name, tm)
                if members is not None:
                    assert tm["track_members"] == members, (dtype, name, tm)
                _check(got, done, want, tag=(dtype, name))
            finally:
                rec.free()


# ---- entry paths of an int8 record on both sides of the bound ------------------------------------------------------

@pytest.fixture(scope="module")
def big_file(tmp_path_factory):
    """name -> (path, record): a BIG_FILE_BYTES file whose first stretch is the int8 record, repeated to the end (one
    file at a time on disk)."""
    m = pkg()
    s = m.Settings()
    d = tmp_path_factory.mktemp("full_scale")
    made = {}

    def get(name):
        if name not in made:
            for path, _ in made.values():
                os.remove(path)
            made.clear()
            x = fsr.int8_records(m, s, MS)[name][0]
            path = str(d / (name + ".bin"))
            with open(path, "wb") as f:
                for _ in range(BIG_FILE_BYTES // x.size + 1):
                    x.tofile(f)
            made[name] = (path, x)
        return made[name]
    yield get
    for path, _ in made.values():
        os.remove(path)


ENTRIES = ["resident", "streamed", "stream_off", "stalled", "track_open", "queued_resident", "queued_file"]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["clean%d" % a for a in fsr.INT8_BELOW + fsr.INT8_ABOVE])
def test_every_entry_path_of_a_strong_int8_record(name, entry, big_file, capfd):
    """The same int8 record through every way it reaches the tracking kernels: resident (ctx.upload), a file streamed in
    beside the kernel (ctx.open_file; track_streamed == 1), the same file with SGX_TRK_STREAM=0 and with the stall hook
    SGX_TRK_TEST_STALL=1 (launches that do not stream, on a record that was still loading when tracking began), the
    reference's own sequence TrackingResult.track(open(path, 'rb')), and the queued step (deferred acquisition ->
    preRun -> DeviceFile) on a resident record and on the file.  The file is 128 MB of which 50 ms are tracked, so that
    the record is normally still loading when tracking starts - which the test cannot observe directly (the streaming
    case's track_streamed, or its repeat's stderr line, says it was there).  Every path runs the kernel the resident
    record runs: 5, or 2 with the stderr line."""
    m = pkg()
    path, raw = big_file(name)
    s, so = _settings(m, "int8")
    keep = _v3_expect(name, "int8")
    kernel = 5 if keep else 2
    ctx = m.engine.get_context(s, 0)
    chans, table = _chans([fsr.clean_channel(s)], 1)
    want = _oracle(so, table, raw)
    n_file = os.path.getsize(path)
    capfd.readouterr()
    if entry in ("resident", "streamed", "stream_off", "stalled"):
        env = {"stream_off": {"SGX_TRK_STREAM": "0"}, "stalled": {"SGX_TRK_TEST_STALL": "1"}}.get(entry, {})
        rec = ctx.upload(raw) if entry == "resident" else ctx.open_file(path, 0, n_file)
        try:
            got, done = _run(ctx, rec, chans, MS, m._native.DT_INT8, env)
        finally:
            rec.free()
        tm, err = _ran(ctx, capfd, kernel, (name, entry))
        assert (TOO_STRONG in err) == (not keep), (name, entry, err)
        if not keep and name in ABOVE and entry != "streamed":
            # a launch that does not stream: the host's magnitude scan sends the record away BEFORE the speculative kernel
            # runs (not the kernel's own look at its prompt sums after a launch, which misses sums that have wrapped)
            assert SCAN_LINE in err, (name, entry, err)
        if entry == "streamed":
            # the launch streamed - or a streaming launch found the record too strong and the repeat on the resident
            # record (track_streamed 0: the last launch's) said so
            assert tm["track_streamed"] == 1 or "repeating the launch with the round-3 kernel" in err, (name, tm, err)
        _check(got, done, want, tag=(name, entry))
    elif entry == "track_open":
        # the reference's call sequence on a file on disk
        a = m.AcquisitionResult(s, device=0)
        a._channels = np.rec.fromarrays([table["PRN"], table["acquiredFreq"], table["codePhase"], ['T']],
                                        names='PRN,acquiredFreq,codePhase,status')
        t = m.TrackingResult(a, device=0)
        with open(path, "rb") as fid:
            t.track(fid)
            assert fid.tell() == int(want[-1, 0, MS - 1])
        _, err = _ran(ctx, capfd, kernel, (name, entry))
        assert (TOO_STRONG in err) == (not keep), (name, entry, err)
        _check(t.series, np.full(1, MS), want, tag=(name, entry))
    else:
        # the queued step: deferred acquisition -> preRun -> DeviceFile
        resident = entry == "queued_resident"
        n = s.samplesPerCode
        rec = ctx.upload(raw) if resident else ctx.open_file(path, 0, n_file)
        try:
            sq = m.Settings()
            sq.numberOfChannels, sq.msToProcess, sq.acqSatelliteList = 1, float(MS), list(range(1, 9))
            aq = m.AcquisitionResult(sq, device=0, deferred=True)
            aq.acquire(m.DeviceSignal(rec, 0, 11 * n))
            aq.preRun()
            tq = m.TrackingResult(aq, device=0)
            tq.track(m.DeviceFile(rec))
        finally:
            rec.free()
        if resident:
            assert tq.chained, name
        _, err = _ran(m.engine.get_context(sq, 0), capfd, kernel, (name, entry))
        assert (TOO_STRONG in err) == (not keep), (name, entry, err)
        if resident and name in ABOVE:
            assert SCAN_LINE in err, (name, entry, err)
        ch = aq.channels
        assert int(ch.PRN[0]) == 5
        soq = orc.OracleSettings(numberOfChannels=1, msToProcess=float(MS))
        wq = orc.stack_series(orc.track(soq, dict(PRN=np.array(ch.PRN), acquiredFreq=np.array(ch.acquiredFreq),
                                                  codePhase=np.array(ch.codePhase), status=['T']), raw))
        _check(tq.series, np.full(1, MS), wq, tag=(name, entry))
