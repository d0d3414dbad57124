"""Multi-correlator replay on the GPU (sgx_track_replay, csrc/sgx_replay.hip) against the reference's own correlator
outputs, the numpy contract of tests/replay_spec.py and the tracking kernels' own arms.  The bar is the project's bar for
correlator series (tests/test_gpu_parity.py): 1e-6 max(1, RMS sqrt(I_P^2 + Q_P^2)) per channel, on EVERY entry - there is no
feedback in a replay, so no entry is excused as a near-boundary sample.  Run with -m gpu."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import replay_cases as cases
import replay_spec as spec
from conftest import ROOT, load_golden, pkg

pytestmark = pytest.mark.gpu

TOL = 1e-6


def _err(got, want, series):
    """max |delta| over the channel's bar 1e-6 max(1, RMS |P|), in units of 1e-6 (so the assertion is < TOL)."""
    worst = 0.0
    for c in range(want.shape[0]):
        scale = max(1.0, float(np.sqrt(np.mean(series[c, 3] ** 2 + series[c, 7] ** 2))))
        worst = max(worst, float(np.max(np.abs(got[c] - want[c]))) / scale)
    return worst


def _report(capsys, what, err):
    with capsys.disabled():
        print("\n[replay] %s: max error %.3g of RMS|P| (bar %.0e)" % (what, err, TOL))


def _settings(m, ms, nch=8):
    s = m.Settings()
    s.msToProcess = float(ms)
    s.numberOfChannels = nch
    return s


def _track(m, s, rec):
    a = m.AcquisitionResult(s, device=0)
    a.acquire(m.DeviceSignal(rec, 0, 11 * s.samplesPerCode))
    a.preRun()
    t = m.TrackingResult(a, device=0)
    t.track(m.DeviceFile(rec))
    chans = [(int(c.PRN), float(c.acquiredFreq), float(c.codePhase)) for c in a.channels if c.PRN != 0]
    return a, t, chans


@pytest.fixture(scope="module")
def run400():
    """The default scene, 8 channels x 400 ms tracked on the GPU, and the record's host copy."""
    m = pkg()
    s = _settings(m, 400)
    ctx = m.engine.get_context(s, 0)
    rec = ctx.synth(m.synth.Scene.default(), m.synth.record_length(s.samplesPerCode, 400))
    a, t, chans = _track(m, s, rec)
    assert t.series.shape == (8, 13, 400) and len(chans) == 8
    yield m, s, ctx, rec, rec.download(), a, t, chans
    rec.free()


def test_reference_anchor(default_record, capsys):
    """The golden series of the reference and its record: taps (-0.5, 0, 0.5) against the reference's I_E .. Q_L."""
    m = pkg()
    so, rec_host, dt, chans, series = cases.case_default(default_record)
    s = _settings(m, 400, 4)
    ctx = m.engine.get_context(s, 0)
    rec = ctx.upload(rec_host)
    try:
        got = ctx.track_replay(rec, chans, series, (-0.5, 0.0, 0.5))
    finally:
        rec.free()
    want = cases.arms(series)
    assert got.shape == want.shape == (4, 3, 2, 400)
    err = _err(got, want, series)
    _report(capsys, "reference anchor, 4 x 400 ms x 3 taps", err)
    assert err < TOL


IRREGULAR = (0.1, -0.37, 1.5 + 1023, -1023.25)


def test_bank_of_21_taps_against_the_contract(run400, capsys):
    m, s, ctx, rec, host, a, t, chans = run400
    taps = list(np.arange(-2.0, 2.01, 0.25)) + list(IRREGULAR)
    assert len(taps) == 21
    got = ctx.track_replay(rec, chans, t.series, taps)
    want, _ = spec.replay_channels(s, host, "int8", chans, t.series, None, taps)
    err = _err(got, want, t.series)
    _report(capsys, "8 x 400 ms x 21 taps against the contract", err)
    assert err < TOL
    # two identical calls give identical bytes
    again = ctx.track_replay(rec, chans, t.series, taps)
    assert got.tobytes() == again.tobytes()


def test_self_consistency_with_the_headline_kernel(capsys):
    """8 x 4 000 ms tracked by the headline kernel, replayed at (-s, 0, +s): the tracking output's own six rows."""
    m = pkg()
    s = _settings(m, 4000)
    ctx = m.engine.get_context(s, 0)
    rec = ctx.synth(m.synth.Scene.default(), m.synth.record_length(s.samplesPerCode, 4000))
    try:
        a, t, chans = _track(m, s, rec)
        assert ctx.timing()["track_kernel"] == 5
        d = s.dllCorrelatorSpacing
        track_ms = ctx.timing()["track_ms"]
        got = ctx.track_replay(rec, chans, t.series, (-d, 0.0, d))
        again = ctx.track_replay(rec, chans, t.series, (-d, 0.0, d))      # (the first call warmed the kernel up)
        kernel_ms, device_ms = ctx.replay_timing()
    finally:
        rec.free()
    err = _err(got, cases.arms(t.series), t.series)
    _report(capsys, "8 x 4 000 ms against the tracking kernel's arms", err)
    assert err < TOL and got.tobytes() == again.tobytes()
    # a replay has no chain: it must take less device time than the tracking launch that produced the series
    with capsys.disabled():
        print("[replay] 8 x 4 000 ms x 3 taps: kernel %.3f ms, device side %.3f ms; tracking launch %.3f ms" % (kernel_ms, device_ms, track_ms))
    assert 0 < kernel_ms <= device_ms < track_ms


def test_uint8_record_and_edge_forms(run400, capsys):
    """uint8 bytes; a channel that is off; ms_done < ms for one channel; 64 taps; 1 tap."""
    m, s, ctx, rec, host, a, t, chans = run400
    ms = 40
    recu = (host[:m.synth.record_length(s.samplesPerCode, ms)].astype(np.int16) + 128).astype(np.uint8)
    so = spec.orc.OracleSettings(numberOfChannels=3, msToProcess=float(ms), dataType='uint8')
    ch3 = dict(PRN=np.array([c[0] for c in chans[:3]]), acquiredFreq=np.array([c[1] for c in chans[:3]]),
               codePhase=np.array([c[2] for c in chans[:3]]), status=['T'] * 3)
    series = spec.orc.stack_series(spec.orc.track(so, ch3, recu))
    du = ctx.upload_bytes(recu)
    try:
        taps64 = np.linspace(-3.0, 3.3, 64)
        got = ctx.track_replay(du, chans[:3], series, taps64, data_type=m._native.DT_UINT8)
        want, _ = spec.replay_channels(so, recu, "uint8", chans[:3], series, None, taps64)
        err = _err(got, want, series)
        _report(capsys, "uint8, 3 x 40 ms x 64 taps", err)
        assert got.shape == (3, 64, 2, ms) and err < TOL
    finally:
        du.free()
    # int8: channel 1 off, channel 2 cut short, one tap
    some = [chans[0], (0, 0.0, 0.0), chans[2], chans[3]]
    ser = np.array(t.series[:4, :, :ms])
    done = np.array([ms, ms, 17, ms], dtype=np.int32)
    for taps in ((0.3,), (-0.5, 0.0, 0.5, 0.75, 1.0)):
        got = ctx.track_replay(rec, some, ser, taps, ms_done=done)
        want, _ = spec.replay_channels(s, host, "int8", some, ser, done, taps)
        assert got.shape == (4, len(taps), 2, ms)
        assert not np.any(got[1]) and not np.any(got[2, :, :, 17:]) and np.any(got[2, :, :, :17])
        err = _err(got, want, ser)
        _report(capsys, "a channel off, a channel cut short, %d taps" % len(taps), err)
        assert err < TOL


def test_int16_records_with_channels_on_odd_bytes(capsys):
    """The reference's two int16 cases, and three channels of which two start on an odd byte (inside a sample), tracked
    by the oracle for 40 ms."""
    m = pkg()
    g = load_golden("trk_int16.npz")
    todo = cases.cases_int16()
    rec16 = todo[0][1]
    prn = np.array([int(g["locked_PRN"][0])] * 3)
    freq = np.array([float(g["locked_acquiredFreq"][0])] * 3)
    phase = np.array([12345.0, 2 * 12346.0, 7.0])
    so = spec.orc.OracleSettings(numberOfChannels=3, msToProcess=40.0, dataType='int16', skipNumberOfBytes=0)
    odd = spec.orc.stack_series(spec.orc.track(so, dict(PRN=prn, acquiredFreq=freq, codePhase=phase, status=['T'] * 3), rec16))
    todo.append((so, rec16, "<i2", cases.chans_of(prn, freq, phase), odd))
    for so, rec16, dt, chans, series in todo:
        s = _settings(m, series.shape[2], len(chans))
        s.dataType = 'int16'
        s.skipNumberOfBytes = so.skipNumberOfBytes
        ctx = m.engine.get_context(s, 0)
        rec = ctx.upload_bytes(rec16)
        try:
            taps = (-0.5, 0.0, 0.5, 0.2)
            got = ctx.track_replay(rec, chans, series, taps, data_type=m._native.DT_INT16)
        finally:
            rec.free()
        want, _ = spec.replay_channels(so, rec16, "<i2", chans, series, None, taps)
        assert _err(got[:, :3], cases.arms(series), series) < TOL        # the reference's / the oracle's own arms
        err = _err(got, want, series)
        _report(capsys, "int16, %d channels from bytes %s" % (len(chans), [int(so.skipNumberOfBytes + c[2]) for c in chans]), err)
        assert err < TOL


def test_second_front_end(capsys):
    m = pkg()
    so, rec_host, dt, chans, series = cases.case_rate2()
    s = _settings(m, series.shape[2], 3)
    s.samplingFreq = 16367600.0
    s.IF = 4130400.0
    ctx = m.engine.get_context(s, 0)
    rec = ctx.upload(rec_host)
    try:
        taps = (-0.5, 0.0, 0.5, -1.1, 0.25)
        got = ctx.track_replay(rec, chans, series, taps)
    finally:
        rec.free()
    want, _ = spec.replay_channels(so, rec_host, "int8", chans, series, None, taps)
    assert _err(got[:, :3], cases.arms(series), series) < TOL
    err = _err(got, want, series)
    _report(capsys, "16.3676 Msps front end, 3 x 250 ms x 5 taps", err)
    assert err < TOL


def test_many_channels(run400, capsys):
    """512 channels x 100 ms, the eight channels repeated whole code periods apart (as the throughput bench leg does),
    against the contract on a sample of 16 channels."""
    m, s, ctx, rec, host, a, t, chans = run400
    n = s.samplesPerCode
    many = [(chans[i % 8][0], chans[i % 8][1], chans[i % 8][2] + (i // 8) * n) for i in range(512)]
    series, done = ctx.track(rec, many, 100)
    assert np.all(done == 100)
    taps = (-0.5, 0.0, 0.5, 0.125, -1.0)
    got = ctx.track_replay(rec, many, series, taps)
    assert got.shape == (512, 5, 2, 100)
    assert _err(got[:, :3], cases.arms(series), series) < TOL            # every channel against its own tracked arms
    picks = [0, 7, 8, 63, 64, 100, 127, 128, 255, 256, 300, 383, 384, 450, 510, 511]
    want, _ = spec.replay_channels(s, host, "int8", [many[i] for i in picks], series[picks], None, taps)
    err = _err(got[picks], want, series[picks])
    _report(capsys, "512 x 100 ms, 16 channels against the contract", err)
    assert err < TOL


def test_bad_arguments_are_refused_and_write_nothing(run400):
    m, s, ctx, rec, host, a, t, chans = run400
    n = m._native
    ser = np.ascontiguousarray(t.series[:, :, :50])
    good = (-0.5, 0.0, 0.5)

    def refused(code, series=ser, taps=good, ms_done=None, data_type=0, ch=chans, rec_off=0):
        tp = np.ascontiguousarray(taps, dtype=np.float64)
        out = np.full((len(ch), max(tp.size, 1), 2, series.shape[2]), 7.0)
        arr = n._chan_array(ch)
        done = None if ms_done is None else np.ascontiguousarray(ms_done, dtype=np.int32)
        rc = n.lib().sgx_track_replay(ctx._h, rec._h, rec_off, C.cast(arr, C.c_void_p), len(ch), series.shape[2],
                                      None if done is None else n._ptr(done), n._ptr(series), data_type, n._ptr(tp),
                                      tp.size, n._ptr(out))
        assert rc == code, (rc, n.last_error())
        assert np.all(out == 7.0)

    refused(n.SGX_E_ARG, taps=np.zeros(0))
    refused(n.SGX_E_ARG, taps=np.zeros(65))
    refused(n.SGX_E_ARG, taps=(0.0, float("nan")))
    refused(n.SGX_E_ARG, taps=(float("inf"),))
    refused(n.SGX_E_ARG, ms_done=[50] * 7 + [51])
    refused(n.SGX_E_ARG, ms_done=[-1] + [50] * 7)
    for dt in (n.DT_FLOAT32, n.DT_FLOAT64, n.DT_UINT16, n.DT_INT32, n.DT_INT64, n.DT_FLOAT16, 77):
        refused(n.SGX_E_ARG, data_type=dt)
    moved = np.array(ser)
    moved[5, 0, 20] -= 1.0
    refused(n.SGX_E_ARG, series=moved)
    refused(n.SGX_E_RANGE, rec_off=int(min(c[2] for c in chans)) + 1)     # the record begins after a channel's start
    L = n.lib()
    arr = n._chan_array(chans)
    tp = np.array(good)
    out = np.full((8, 3, 2, 50), 7.0)
    args = [ctx._h, rec._h, 0, C.cast(arr, C.c_void_p), 8, 50, None, n._ptr(ser), 0, n._ptr(tp), 3, n._ptr(out)]
    for i in (0, 1, 3, 7, 9, 11):
        bad = list(args)
        bad[i] = None
        assert L.sgx_track_replay(*bad) == n.SGX_E_ARG
    assert np.all(out == 7.0)
    assert L.sgx_track_replay(*args) == n.SGX_OK and not np.any(out == 7.0)
    # a record shorter than the series needs
    short = ctx.upload(host[:int(ser[:, 0, -1].max()) - 1])
    try:
        with pytest.raises(n.SgxError) as e:
            ctx.track_replay(short, chans, ser, good)
        assert e.value.code == n.SGX_E_RANGE
    finally:
        short.free()


def test_tracking_result_replay_end_to_end(run400, capsys):
    m, s, ctx, rec, host, a, t, chans = run400
    d = s.dllCorrelatorSpacing
    r = t.replay(m.DeviceFile(rec), (-d, 0.0, d))
    assert r.I.shape == r.Q.shape == (8, 3, 400) and list(r.taps) == [-d, 0.0, d]
    assert list(r.PRN) == [c[0] for c in chans]
    want = cases.arms(t.series)
    got = np.stack([r.I, r.Q], axis=2)
    assert _err(got, want, t.series) < TOL
    assert np.array_equal(r.envelope(), np.sqrt(r.I ** 2 + r.Q ** 2))
    assert np.all(np.argmax(r.envelope()[:, :, 100:].mean(axis=2), axis=1) == 1)
    # ... and when .results was assigned from a cache (the reference's path), from a real file
    t2 = m.TrackingResult(a, device=0)
    t2.results = t.results
    r2 = t2.replay(m.DeviceFile(rec), (-d, 0.0, d))
    assert r2.I.tobytes() == r.I.tobytes() and r2.Q.tobytes() == r.Q.tobytes()


def test_command_line_correlator_bank(run400, tmp_path):
    m, s, ctx, rec, host, a, t, chans = run400
    path = str(tmp_path / "record.bin")
    host[:m.synth.record_length(s.samplesPerCode, 80)].tofile(path)
    r = subprocess.run([sys.executable, "-m", "softgnss-python_amd.main", path, "--ms", "60", "--no-probe",
                        "--correlator-bank=-1:1:0.5"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=600, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "Correlator bank (5 taps" in r.stdout
    rows = [ln.split("|") for ln in r.stdout.splitlines() if ln.startswith("|") and ln.count("|") == 5 and "tap" not in ln]
    rows = [(int(x[1]), int(x[2]), float(x[3]), float(x[4])) for x in rows]
    assert len(rows) == 8 * 5
    for c in range(8):
        env = [x[3] for x in rows if x[0] == c]
        assert [x[2] for x in rows if x[0] == c] == [-1.0, -0.5, 0.0, 0.5, 1.0]
        assert env[2] == 1.0 and env[0] < 0.3 and env[4] < 0.3 and 0.3 < env[1] < 0.8 and 0.3 < env[3] < 0.8, env
