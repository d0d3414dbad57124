"""GPU: sgx_track_coherent (csrc/sgx_trk_coh.hip) against its numpy contract (tests/coh_track_spec.py) on the scenes of
tests/coh_track_cases.py.  The bar is the project's tracking bar: absoluteSample, ms_done, the bit edge and k0 exactly; the
other twelve series within 1e-9 of each series' scale; the bit-synchronisation energies within 1e-9 relative."""
import numpy as np
import pytest

import coh_track_cases as cases
import coh_track_spec as spec
from conftest import load_golden, pkg

pytestmark = pytest.mark.gpu

TOL = 1e-9
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _settings(m, s, **kw):
    """The package's Settings for an oracle settings object."""
    p = m.Settings()
    p.samplingFreq, p.IF = s.samplingFreq, s.IF
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _trk_err(got, want, done):
    """The largest |delta| over its bar's scale: the six correlator series over max(1, RMS sqrt(I_P^2 + Q_P^2)) per channel
    (tests/test_gpu_parity.py), each other series over the largest finite magnitude it takes in that channel.  Entries that
    are not finite (the pre-fill, a silent update's NaN) must be the same on both sides."""
    worst = 0.0
    for c in range(want.shape[0]):
        n = int(done[c])
        assert np.array_equal(got[c, :, n:], want[c, :, n:]), "the pre-fill behind ms_done"
        if n == 0:
            continue
        g, w = got[c, :, :n], want[c, :, :n]
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w))
        rms = max(1.0, float(np.sqrt(np.mean(w[3] ** 2 + w[7] ** 2))))
        for k in range(1, 13):
            fin = np.isfinite(w[k])
            if not fin.any():
                continue
            scale = rms if 3 <= k <= 8 else float(np.max(np.abs(w[k][fin])))
            worst = max(worst, float(np.max(np.abs(g[k][fin] - w[k][fin]))) / scale if scale > 0 else 0.0)
    return worst


def _same(got, want):
    """got: (series, ms_done, edge, k0, energy) of Context.track_coherent; want: the spec's dict."""
    series, done, edge, k0, energy = got
    assert np.array_equal(done, want["ms_done"])
    assert np.array_equal(edge, want["edge"]) and np.array_equal(k0, want["k0"])
    assert np.array_equal(series[:, 0], want["series"][:, 0])
    err = _trk_err(series, want["series"], done)
    print("\n[coherent tracking] max error %.3g of the series' scale (bar %.0e)" % (err, TOL))
    assert err < TOL
    assert np.allclose(energy, want["energy"], rtol=1e-9, atol=0.0)


def _run(m, s, rec_host, chans, ms, T, P, H, edges, **loops):
    ps = _settings(m, s, **loops)
    ctx = m.engine.get_context(ps, 0)
    rec = ctx.upload(rec_host)
    try:
        return ctx.track_coherent(rec, chans, ms, m._native.coh_params(ps, T, P, H), bit_edge=edges), ctx
    finally:
        rec.free()


def _trio(ms, fs=cases.FS_LOW, IF=cases.IF_LOW):
    return _once(("trio", ms, fs), lambda: cases.scene_trio(ms, fs, IF))


@pytest.mark.parametrize("fs,IF", [(cases.FS_LOW, cases.IF_LOW), (16.368e6, 4.1304e6)])
def test_all_1ms_anchor(fs, IF, monkeypatch):
    """The pull-in as long as the run: the spec, and sgx_track's series on the same channels - within TOL of the kernels
    sgx_track picks by itself, and BIT FOR BIT those of the per-sample body with one member per channel, which runs the
    block pieces the coherent kernel runs (csrc/sgx_trk_block.h): trk_kernel_multi at 4 samples per chip (both take the
    sample-by-sample map), trk_kernel_any on the same values as an int32 record at 16 samples per chip (both take the
    one-switch map; positions are bytes there)."""
    m = pkg()
    ms = 300
    s, rec, chans, edges = _trio(ms, fs, IF)
    chans, edges = chans[:2], edges[:2]
    want = spec.track(s, chans, rec, ms, 20, ms, 100, edges)
    got, ctx = _run(m, s, rec, chans, ms, 20, ms, 100, edges)
    _same(got, want)
    assert ctx.timing()["track_kernel"] == 7.0
    dev = ctx.upload(rec)
    try:
        plain, done = ctx.track(dev, chans, ms)
    finally:
        dev.free()
    assert np.array_equal(done, got[1]) and np.array_equal(plain[:, 0], got[0][:, 0])
    assert _trk_err(got[0], plain, done) < TOL
    monkeypatch.setenv("SGX_TRK_SPLIT", "1")       # (read at each call: one workgroup per channel)
    low = fs == cases.FS_LOW
    dev = ctx.upload(rec) if low else ctx.upload_bytes(rec.astype('<i4'))
    try:
        if low:
            one, done = ctx.track(dev, chans, ms)
        else:
            one, done = ctx.track(dev, [(prn, f, 4 * cp) for prn, f, cp in chans], ms, data_type=m._native.DT_INT32)
            assert np.all(one[:, 0] % 4 == 0)
            one = one.copy()
            one[:, 0] /= 4                         # absoluteSample: bytes of the int32 record -> samples
    finally:
        dev.free()
    t = ctx.timing()
    assert t["track_kernel"] == (4 if low else 6) and t["track_members"] == 1
    assert np.array_equal(done, got[1])
    assert np.array_equal(one, got[0], equal_nan=True)


@pytest.mark.parametrize("T", [2, 4, 5, 10, 20])
def test_group_logic_with_given_edges(T):
    """Edges 0, 7 and 19 and a channel that is off; the hand-over window reaches back to block 0 (H > k0) and ms cuts the
    last group of some channels."""
    m = pkg()
    ms, P, H = 110, 40, 100
    s, rec, chans, edges = _trio(400)
    want = spec.track(s, chans, rec, ms, T, P, H, edges)
    assert list(want["k0"]) == [40, 47, 59, -1] and list(want["ms_done"]) == [ms, ms, ms, 0]
    got, _ = _run(m, s, rec, chans, ms, T, P, H, edges)
    _same(got, want)


@pytest.mark.parametrize("P", [P for P, skip in cases.SYNC_SCENES if skip == 0])
def test_bit_sync_in_the_kernel(P):
    """The edges are found (P = 300, 307, 308): k0 = P for the edge-7 channel at P = 307, P + 19 at P = 308."""
    m = pkg()
    ms = cases.SYNC_MS
    s, rec, chans, edges = _trio(ms)
    want = _once(("sync", P), lambda: spec.track(s, chans, rec, ms, 20, P, 100, [-1] * 4))
    assert list(want["edge"][:3]) == edges[:3]
    got, _ = _run(m, s, rec, chans, ms, 20, P, 100, [-1] * 4)
    _same(got, want)


def test_default_front_end(default_record):
    """38.192 Msps (one chip switch per ramp and group of 16 samples), the default scene's first two channels."""
    m = pkg()
    g = load_golden("trk_default.npz")
    ms = 400
    s = cases.settings(38.192e6, 9.548e6)
    chans = [(int(g["ch_PRN"][i]), float(g["ch_acquiredFreq"][i]), float(g["ch_codePhase"][i])) for i in range(2)]
    want = spec.track(s, chans, default_record, ms, 10, 300, 100, [3, 11])
    assert list(want["ms_done"]) == [ms, ms] and list(want["k0"]) == [303, 311]
    got, _ = _run(m, s, default_record, chans, ms, 10, 300, 100, [3, 11])
    _same(got, want)


def _tracker(m, ps, chans):
    a = m.AcquisitionResult(ps, device=0)
    n = len(chans)
    a._channels = np.rec.fromarrays([[c[0] for c in chans], [c[1] for c in chans], [c[2] for c in chans],
                                     ['T' if c[0] else '-' for c in chans]], names='PRN,acquiredFreq,codePhase,status')
    ps.numberOfChannels = n
    return m.TrackingResult(a, device=0)


@pytest.mark.parametrize("H", [1, 37, 1000])
def test_hand_over_windows(H):
    """One value, a ring that has wrapped at a length that does not divide k0, and the longest window (H' = k0)."""
    m = pkg()
    ms, P = 110, 60
    s, rec, chans, edges = _trio(400)
    want = spec.track(s, chans, rec, ms, 4, P, H, edges)
    assert list(want["k0"]) == [60, 67, 79, -1]
    got, _ = _run(m, s, rec, chans, ms, 4, P, H, edges)
    _same(got, want)


def test_record_file_through_track(tmp_path):
    """TrackingResult.track on a file on disk with skipNumberOfBytes: the record is loaded as the 1 ms path loads it."""
    m = pkg()
    (P, skip), = [e for e in cases.SYNC_SCENES if e[1]]          # P = 260 behind 1000 bytes: a scene with a margin
    ms = cases.SYNC_MS
    s, padded, chans, edges = cases.scene_sync(skip)
    want = spec.track(s, chans, padded, ms, 20, P, 100, [-1] * 4)
    assert list(want["edge"][:3]) == edges[:3]
    ps = _settings(m, s, trackCoherentMs=20, trackPullInMs=P, msToProcess=float(ms), skipNumberOfBytes=skip)
    t = _tracker(m, ps, chans)
    name = str(tmp_path / "trio.bin")
    padded.tofile(name)
    with open(name, "rb") as fid:
        t.track(fid)
        assert fid.tell() == int(want["series"][2, 0, ms - 1])
    pick = {k: v[:3] for k, v in want.items()}
    _same((t.series, np.full(3, ms, dtype=np.int32), t.bitEdge, t.coherentStart, t.edgeEnergy), pick)


def test_short_record(capsys):
    """The record ends inside the third 20 ms group of channel 0."""
    m = pkg()
    ms, P, H = 110, 40, 100
    s, rec, chans, edges = _trio(400)
    cut = rec[:int(chans[0][2]) + 92 * 4092 + 100]
    want = spec.track(s, chans, cut, ms, 20, P, H, edges)
    assert 80 < want["ms_done"][0] < 100 and np.all(want["ms_done"][:3] < ms)
    got, _ = _run(m, s, cut, chans, ms, 20, P, H, edges)
    _same(got, want)
    ps = _settings(m, s, trackCoherentMs=20, trackPullInMs=220, msToProcess=300.0)
    t = _tracker(m, ps, chans)
    ctx = m.engine.get_context(ps, 0)
    short = rec[:int(chans[0][2]) + 270 * 4092]
    fid = m.DeviceFile(ctx.upload(short))
    try:
        assert t.track(fid) is None and not t.has_results()
    finally:
        fid.record.free()
    assert "Not able to read the specified number of samples for tracking, exiting!" in capsys.readouterr().out


def test_silence():
    """Zeros from a point inside the coherent phase: every channel ends behind the first group that is all zeros."""
    m = pkg()
    ms, P, H = 200, 40, 100
    s, rec, chans, edges = _trio(400)
    quiet = rec.copy()
    quiet[int(chans[0][2]) + 70 * 4092:] = 0
    want = spec.track(s, chans, quiet, ms, 20, P, H, edges)
    assert np.all(want["ms_done"][:3] < ms) and np.all(want["ms_done"][:3] > 80)
    ps = _settings(m, s)
    ctx = m.engine.get_context(ps, 0)
    dev = ctx.upload(quiet)
    try:
        with pytest.raises(ValueError, match="channel 0 went silent") as info:
            ctx.track_coherent(dev, chans, ms, m._native.coh_params(ps, 20, P, H), bit_edge=edges)
        e = info.value
        assert isinstance(e, m._native.SilentChannelError) and e.code == m._native.SGX_E_SILENT
        _same((e.series, e.ms_done, e.bit_edge, e.coh_start, e.edge_energy), want)
        last = int(e.ms_done[0]) - 1
        assert np.isnan(e.series[0, 1, last]) and np.all(e.series[0, 3:9, last] == 0.0)
        ps2 = _settings(m, s, trackCoherentMs=20, trackPullInMs=220, msToProcess=400.0)
        quiet2 = rec.copy()
        quiet2[int(chans[0][2]) + 290 * 4092:] = 0
        dev2 = ctx.upload(quiet2)
        try:
            with pytest.raises(ValueError, match="went silent"):
                _tracker(m, ps2, chans).track(m.DeviceFile(dev2))
        finally:
            dev2.free()
    finally:
        dev.free()


@pytest.fixture(scope="module", params=[1, 2])
def fade(request):
    """Scene F through Settings.trackCoherentMs = 20 and TrackingResult.track."""
    m = pkg()
    s, rec, bits, ch = cases.scene_f(request.param)
    ps = _settings(m, s, trackCoherentMs=20, trackPullInMs=600, trackHandOverMs=100, msToProcess=float(cases.F_MS))
    t = _tracker(m, ps, [ch])
    ctx = m.engine.get_context(ps, 0)
    dev = ctx.upload(rec)
    fid = m.DeviceFile(dev)
    t.track(fid)
    yield m, s, rec, bits, ch, t, fid
    dev.free()


def test_fade_scene_end_to_end(fade):
    m, s, rec, bits, ch, t, fid = fade
    want = spec.track(s, [ch], rec, cases.F_MS, 20, 600, 100, [-1])
    _same((t.series, np.array([cases.F_MS]), t.bitEdge, t.coherentStart, t.edgeEnergy), want)
    assert t.bitEdge[0] == cases.F["edge"] and t.coherentStart[0] == 607 and t.edgeEnergy.shape == (1, 20)
    assert len(t.results) == 1 and int(t.results[0].PRN) == cases.F["prn"]
    assert cases.wrong_bits(t.series[0, 3], bits, cases.F["edge"], cases.F_MS - 1500) == 0.0
    assert np.max(np.abs(t.series[0, 2, -1000:] - (cases.IF_LOW + cases.F["doppler"]))) < 10.0
    # the default settings on the same record: the 1 ms loops have lost the carrier (what the feature is for)
    ps = _settings(m, s, msToProcess=float(cases.F_MS))
    plain = _tracker(m, ps, [ch])
    plain.track(fid)
    assert plain.bitEdge is None
    assert cases.wrong_bits(plain.series[0, 3], bits, cases.F["edge"], cases.F_MS - 1500) >= 0.20


def test_downstream_reads_the_result_unchanged(fade):
    m, s, rec, bits, ch, t, fid = fade
    got = t.replay(fid, [0.0])
    rms = max(1.0, float(np.sqrt(np.mean(t.series[0, 3] ** 2 + t.series[0, 7] ** 2))))
    err = max(np.max(np.abs(got.I[0, 0] - t.series[0, 3])), np.max(np.abs(got.Q[0, 0] - t.series[0, 7]))) / rms
    print("\n[coherent tracking] replay of the prompt tap: max error %.3g of RMS|P| (bar 1e-6)" % err)
    assert err < 1e-6                              # the bar of tests/test_replay_gpu.py
    q = t.quality
    assert len(q) == 1 and int(q[0].PRN) == cases.F["prn"] and int(q[0].lostAtMs) == -1


def test_determinism_and_arguments():
    m = pkg()
    ms = 110
    s, rec, chans, edges = _trio(400)
    a, ctx = _run(m, s, rec, chans, ms, 10, 40, 100, edges)
    b, _ = _run(m, s, rec, chans, ms, 10, 40, 100, edges)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    n = m._native
    ps = _settings(m, s)
    dev = ctx.upload(rec)
    try:
        ctx.track(dev, chans, 5)               # a plain sgx_track: it leaves its own kernel number in the timing
        before = ctx.timing()
        assert before["track_kernel"] != 7.0

        def refused(T=20, P=40, H=100, e=edges, run_ms=ms):
            with pytest.raises(n.SgxError) as info:
                ctx.track_coherent(dev, chans, run_ms, n.coh_params(ps, T, P, H), bit_edge=e)
            assert info.value.code == n.SGX_E_ARG
            assert ctx.timing() == before          # nothing was launched: a launch writes track_kernel = 7 and its time
        for T in (0, 3, 8, 40):
            refused(T=T)
        refused(P=39)
        refused(P=219, e=[-1, 7, 19, 0])
        refused(P=ms + 1)
        refused(P=250, e=[-1, 7, 19, 0], run_ms=240)
        refused(H=0)
        refused(H=1001)
        refused(e=[0, 7, 20, 0])
        refused(e=[0, -2, 19, 0])
        # (an edge to be found on a channel that is off asks nothing of the pull-in)
        ctx.track_coherent(dev, chans, ms, n.coh_params(ps, 20, 40, 100), bit_edge=[0, 7, 19, -1])
        with pytest.raises(TypeError):
            ctx.track_coherent(dev, chans, ms, n.coh_params(ps, 20, 40, 100), bit_edge=edges, data_type=n.DT_INT16)
        with pytest.raises(TypeError):
            _tracker(m, _settings(m, s, trackCoherentMs=20, dataType='int16', msToProcess=300.0), chans).track(m.DeviceFile(dev))
        # trackCoherentMs = 1: track() never reaches the new entry point
        def never(*args, **kw):
            raise AssertionError("Context.track_coherent called at trackCoherentMs = 1")
        old = type(ctx).track_coherent
        type(ctx).track_coherent = never
        try:
            t = _tracker(m, _settings(m, s, msToProcess=60.0), chans)
            t.track(m.DeviceFile(dev))
            assert t.series.shape == (3, 13, 60) and t.bitEdge is None
        finally:
            type(ctx).track_coherent = old
    finally:
        dev.free()
