"""GPU: sgx_track_coherent (csrc/sgx_trk_coh.hip) at its limits and beside the other stages - the cases of
tests/coh_track_cases.py ("the limits"), each shown on the CPU by tests/test_coh_track_cases.py to have its nearest wrong
result outside the bar.  The bar is that of tests/test_coh_track_gpu.py, through its own _same: absoluteSample, ms_done, the
bit edge, k0 and the pre-fill exactly, the other twelve series within 1e-9 of each series' scale, the energies within 1e-9
relative.  Nothing here changes the arithmetic of a block, so nothing gets another number."""
import numpy as np
import pytest

import cancel_spec
import coh_track_cases as cases
import coh_track_spec as spec
from conftest import load_golden, pkg
from test_coh_track_gpu import TOL, _once, _run, _same, _settings, _tracker, _trk_err

pytestmark = pytest.mark.gpu


def _trio():
    return _once(("trio", cases.SYNC_MS, cases.FS_LOW), lambda: cases.scene_trio(cases.SYNC_MS))


def _at_offset(want, off):
    """The contract's result with the record `off` bytes into the file: absoluteSample of every block that ran."""
    out = dict(want, series=want["series"].copy())
    for c, n in enumerate(want["ms_done"]):
        out["series"][c, 0, :int(n)] += off
    return out


# ---- 1. rates -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,IF,T", [(fs, IF, 20) for fs, IF, _, _ in cases.RATE_SCENES] + [(16.368e6, 4.1304e6, 4)])
def test_rates(fs, IF, T):
    """Coherent groups at 5.33, 15, 16 and 60 samples per chip: 2, 4, 5 and 16 units, both maps, and at 16 per chip the
    one-switch map's sample-by-sample route (E, P and L switch 8 samples apart) - there also with groups that end inside a bit."""
    m = pkg()
    run = dict(cases.RATE_RUN, T=T)
    s, rec, chans, edges = _once(("trio", run["ms"], fs), lambda: cases.scene_trio(run["ms"], fs, IF))
    want = spec.track(s, chans, rec, edges=edges, **run)
    assert list(want["k0"]) == [40, 47, 59, -1] and list(want["ms_done"]) == [110, 110, 110, 0]
    got, ctx = _run(m, s, rec, chans, run["ms"], T, run["P"], run["H"], edges)
    _same(got, want)
    assert ctx.timing()["track_kernel"] == 7.0


# ---- 2. a record at an offset ---------------------------------------------------------------------------------------------

def _offset_run(m, s, rec_host, chans, edges, off):
    run = cases.OFFSET_RUN
    ps = _settings(m, s)
    ctx = m.engine.get_context(ps, 0)
    dev = ctx.upload(rec_host)
    try:
        return ctx.track_coherent(dev, chans, run["ms"], m._native.coh_params(ps, run["T"], run["P"], run["H"]), bit_edge=edges,
                                  rec_file_offset=off)
    finally:
        dev.free()


def test_a_window_of_the_file():
    """The record from byte 3 * 4096 of the file on, the channels at their file positions: every sample keeps its place in its
    16-byte group, so the run equals the one on the whole record byte for byte - and the contract."""
    m = pkg()
    s, rec, chans, edges = _trio()
    off = cases.OFFSETS["window"]
    moved, e2 = cases.moved_behind(chans, edges, off)
    want = spec.track(s, moved, rec, edges=e2, **cases.OFFSET_RUN)
    whole = _offset_run(m, s, rec, moved, e2, 0)
    part = _offset_run(m, s, rec[off:], moved, e2, off)
    _same(part, want)
    for a, b in zip(part, whole):
        assert a.tobytes() == b.tobytes()


def test_an_odd_offset():
    """The same from byte 3 * 4096 + 5 on: every sample sits in another place of its group."""
    m = pkg()
    s, rec, chans, edges = _trio()
    off = cases.OFFSETS["odd"]
    moved, e2 = cases.moved_behind(chans, edges, off)
    want = spec.track(s, moved, rec, edges=e2, **cases.OFFSET_RUN)
    _same(_offset_run(m, s, rec[off:], moved, e2, off), want)


def test_a_large_offset():
    """The whole record declared to start at file byte 2^33 + 4096: absoluteSample is the contract's plus that, exactly;
    everything else is the run at offset 0, byte for byte (the offset is a multiple of 16)."""
    m = pkg()
    s, rec, chans, edges = _trio()
    off = cases.OFFSETS["large"]
    want = spec.track(s, chans, rec, edges=edges, **cases.OFFSET_RUN)
    far = _offset_run(m, s, rec, [(p, f, cp + off if p else cp) for p, f, cp in chans], edges, off)
    _same(far, _at_offset(want, off))
    near = _offset_run(m, s, rec, chans, edges, 0)
    assert far[0][:, 1:].tobytes() == near[0][:, 1:].tobytes()
    assert np.array_equal(far[0][:3, 0] - off, near[0][:3, 0]) and np.array_equal(far[0][3, 0], near[0][3, 0])
    for a, b in zip(far[1:], near[1:]):
        assert a.tobytes() == b.tobytes()


def test_a_channel_in_front_of_the_record_is_refused():
    m = pkg()
    n = m._native
    s, rec, chans, edges = _trio()
    off = cases.OFFSETS["window"]
    run = cases.OFFSET_RUN
    ps = _settings(m, s)
    ctx = m.engine.get_context(ps, 0)
    dev = ctx.upload(rec[off:])
    try:
        ctx.track(dev, [(p, f, cp + off if p else cp) for p, f, cp in chans], 5, rec_file_offset=off)
        before = ctx.timing()
        assert before["track_kernel"] != 7.0
        moved, e2 = cases.moved_behind(chans, edges, off)
        early = [moved[0], chans[1], moved[2], moved[3]]                  # channel 1 at byte 1999 of the file
        with pytest.raises(n.SgxError, match="before the record") as info:
            ctx.track_coherent(dev, early, run["ms"], n.coh_params(ps, run["T"], run["P"], run["H"]), bit_edge=e2, rec_file_offset=off)
        assert info.value.code == n.SGX_E_RANGE and "channel 1 " in str(info.value)
        assert ctx.timing() == before              # nothing was launched
        off_row = [moved[0], moved[1], moved[2], (0, 0.0, 0.0)]           # (a row that is off is in front of nothing)
        got = ctx.track_coherent(dev, off_row, run["ms"], n.coh_params(ps, run["T"], run["P"], run["H"]), bit_edge=e2, rec_file_offset=off)
        assert list(got[1]) == [run["ms"]] * 3 + [0]
    finally:
        dev.free()


def test_a_streaming_record_at_an_offset_through_track(tmp_path):
    """TrackingResult.track on a DeviceFile over bytes 8192 .. of a file that is still being read when track() is called:
    the edges are found (P = 300, T = 20), positions are the file's."""
    m = pkg()
    s, rec, chans, edges = _trio()
    off = cases.OFFSETS["classes"]
    run = cases.OFFSET_SYNC
    moved, e2 = cases.moved_behind(chans, edges, off)
    want = _once("classes", lambda: spec.track(s, moved, rec, edges=[-1] * 4, **run))
    assert list(want["edge"][:3]) == e2[:3]
    ps = _settings(m, s, trackCoherentMs=run["T"], trackPullInMs=run["P"], trackHandOverMs=run["H"], msToProcess=float(run["ms"]))
    t = _tracker(m, ps, moved)
    ctx = m.engine.get_context(ps, 0)
    path = str(tmp_path / "trio.bin")
    rec.tofile(path)
    fid = m.DeviceFile(ctx.open_file(path, off, rec.size - off), off)
    try:
        t.track(fid)                               # at once: the record is still streaming in
        assert t.has_results() and fid.tell() == int(want["series"][2, 0, run["ms"] - 1])
    finally:
        fid.record.free()
    pick = {k: v[:3] for k, v in want.items()}
    _same((t.series, np.full(3, run["ms"], dtype=np.int32), t.bitEdge, t.coherentStart, t.edgeEnergy), pick)


# ---- 4. many channels -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_ch", [cases.MANY, 65])
def test_many_channels(n_ch):
    """300 rows - more workgroups than CUs, int arrays of the call that fill five 256-byte slots - and 65, the first size at
    which they fill more than one; rows that are off on both sides of the 64th."""
    m = pkg()
    s, rec, chans, edges = _trio()
    rows, ed = cases.many_channels(chans, edges)
    run = cases.MANY_RUN
    want = _once("many", lambda: spec.track(s, rows, rec, edges=ed, **run))
    want = {k: v[:n_ch] for k, v in want.items()}
    assert sorted(set(want["ms_done"])) == [0, run["ms"]]
    got, _ = _run(m, s, rec, rows[:n_ch], run["ms"], run["T"], run["P"], run["H"], ed[:n_ch])
    _same(got, want)
    for i in cases.MANY_OFF:
        if i < n_ch:
            assert got[1][i] == 0 and got[2][i] == ed[i] and got[3][i] == -1 and np.all(got[4][i] == 0.0)


# ---- 5. full scale ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["clipped", "clean"])
@pytest.mark.parametrize("fs,IF", cases.FULL_SCALE_RATES)
def test_full_scale(fs, IF, kind):
    """Every byte -128 or 127, and a noiseless record at amplitude 127, on both maps."""
    m = pkg()
    s, rec, ch = cases.full_scale_case(m, fs, IF, kind)
    run = cases.FULL_SCALE_RUN
    want = spec.track(s, ch, rec, edges=[cases.FULL_SCALE_EDGE], **run)
    assert list(want["ms_done"]) == [100] and list(want["k0"]) == [43]
    got, _ = _run(m, s, rec, ch, run["ms"], run["T"], run["P"], run["H"], [cases.FULL_SCALE_EDGE])
    _same(got, want)


# ---- 6. T = 1 ---------------------------------------------------------------------------------------------------------------

def test_one_ms_through_the_entry_point():
    """coherent_ms = 1: the edges are found, no coherent phase starts, and the series are sgx_track's."""
    m = pkg()
    s, rec, chans, edges = _trio()
    run = cases.T1_RUN
    want = spec.track(s, chans, rec, edges=[-1] * 4, **run)
    assert list(want["edge"][:3]) == edges[:3] and list(want["k0"]) == [-1] * 4
    got, ctx = _run(m, s, rec, chans, run["ms"], run["T"], run["P"], run["H"], [-1] * 4)
    _same(got, want)
    dev = ctx.upload(rec)
    try:
        plain, done = ctx.track(dev, chans, run["ms"])
    finally:
        dev.free()
    assert np.array_equal(done, got[1]) and np.array_equal(plain[:, 0], got[0][:, 0])
    err = _trk_err(got[0], plain, done)
    print("\n[coherent tracking] T = 1 against sgx_track: max error %.3g of the series' scale (bar %.0e)" % (err, TOL))
    assert err < TOL


# ---- 7. a channel that ends while its edge is sought ------------------------------------------------------------------------

def test_silence_while_the_edge_is_sought():
    m = pkg()
    s, rec, chans, edges = _trio()
    run = cases.ENDS_RUN
    quiet = cases.ends_early(rec, chans, "silence")
    want = spec.track(s, chans, quiet, edges=[-1] * 4, **run)
    assert list(want["ms_done"]) == [101, 101, 101, 0] and list(want["edge"]) == [-1] * 4 and list(want["k0"]) == [-1] * 4
    ps = _settings(m, s)
    ctx = m.engine.get_context(ps, 0)
    dev = ctx.upload(quiet)
    try:
        with pytest.raises(ValueError, match="channel 0 went silent") as info:
            ctx.track_coherent(dev, chans, run["ms"], m._native.coh_params(ps, run["T"], run["P"], run["H"]), bit_edge=[-1] * 4)
    finally:
        dev.free()
    e = info.value
    assert isinstance(e, m._native.SilentChannelError) and e.code == m._native.SGX_E_SILENT
    _same((e.series, e.ms_done, e.bit_edge, e.coh_start, e.edge_energy), want)
    assert list(e.bit_edge) == [-1] * 4 and np.all(e.edge_energy[:3].max(axis=1) > 5e10)
    for c in range(3):
        assert np.isnan(e.series[c, 1, 100]) and np.all(e.series[c, 3:9, 100] == 0.0)


def test_a_short_read_while_the_edge_is_sought():
    m = pkg()
    s, rec, chans, edges = _trio()
    run = cases.ENDS_RUN
    cut = cases.ends_early(rec, chans, "short")
    want = spec.track(s, chans, cut, edges=[-1] * 4, **run)
    assert list(want["ms_done"]) == [150, 149, 149, 0] and list(want["edge"]) == [-1] * 4 and list(want["k0"]) == [-1] * 4
    got, _ = _run(m, s, cut, chans, run["ms"], run["T"], run["P"], run["H"], [-1] * 4)
    _same(got, want)
    assert np.all(got[4][:3].max(axis=1) > 5e10)


# ---- 8. a block beyond the units ------------------------------------------------------------------------------------------

def test_a_block_beyond_the_units_is_an_error_not_a_silent_truncation():
    """tests/test_gpu_parity.py's range test through the coherent kernel's own copy of the check: at 2 kHz the run fits its
    ten units and completes (its loops ride on noise: completion only), at 6 kHz channel 1 reaches a block of 43 120 samples
    and the call says so."""
    m = pkg()
    n = m._native
    run = cases.RANGE_RUN
    for bw, fits in ((2000.0, True), (6000.0, False)):
        ps = m.Settings()
        ps.dllNoiseBandwidth = bw
        ctx = m.engine.get_context(ps, 0)
        rec = ctx.synth(m.synth.Scene.default(), m.synth.record_length(ps.samplesPerCode, 80))
        try:
            params = n.coh_params(ps, run["T"], run["P"], run["H"])
            if fits:
                got = ctx.track_coherent(rec, cases.RANGE_CHANNELS, run["ms"], params, bit_edge=[0, 0])
                assert list(got[1]) == [run["ms"]] * 2 and list(got[3]) == [40, 40]
            else:
                with pytest.raises(n.SgxError, match="plausible range") as info:
                    ctx.track_coherent(rec, cases.RANGE_CHANNELS, run["ms"], params, bit_edge=[0, 0])
                assert info.value.code == n.SGX_E_RANGE and "channel 1 " in str(info.value)
        finally:
            rec.free()


# ---- 9. other loops ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loops", cases.LOOPS, ids=["spacing", "loops"])
def test_other_loops(loops):
    """A quarter-chip spacing, and other 1 ms loops, with coherent loops of 8 and 0.5 Hz: through Settings and coh_params."""
    m = pkg()
    s0, rec, chans, edges = _trio()
    s = cases.settings(**loops)
    run = cases.LOOPS_RUN
    want = spec.track(s, chans, rec, edges=edges, coh_pll_bw=cases.LOOPS_COH["cohPllNoiseBandwidth"],
                      coh_dll_bw=cases.LOOPS_COH["cohDllNoiseBandwidth"], **run)
    assert list(want["ms_done"]) == [150, 150, 150, 0]
    got, _ = _run(m, s, rec, chans, run["ms"], run["T"], run["P"], run["H"], edges, **dict(loops, **cases.LOOPS_COH))
    _same(got, want)


def test_quarter_chip_at_the_default_front_end(default_record):
    """38.192 Msps: a quarter chip is 9.3 samples, so E, P and L can switch inside one group of 16 at different samples."""
    m = pkg()
    g = load_golden("trk_default.npz")
    chans = [(int(g["ch_PRN"][i]), float(g["ch_acquiredFreq"][i]), float(g["ch_codePhase"][i])) for i in range(2)]
    loops = cases.LOOPS[0]
    s = cases.settings(38.192e6, 9.548e6, **loops)
    run = cases.LOOPS_DEFAULT_RUN
    rec = default_record[:(run["ms"] + 3) * 38192 + 38192]
    want = spec.track(s, chans, rec, edges=[3, 11], coh_pll_bw=cases.LOOPS_COH["cohPllNoiseBandwidth"],
                      coh_dll_bw=cases.LOOPS_COH["cohDllNoiseBandwidth"], **run)
    assert list(want["ms_done"]) == [120, 120] and list(want["k0"]) == [43, 51]
    got, _ = _run(m, s, rec, chans, run["ms"], run["T"], run["P"], run["H"], [3, 11], **dict(loops, **cases.LOOPS_COH))
    _same(got, want)


# ---- 10. beside cancellation and the replay ---------------------------------------------------------------------------------

def test_beside_cancellation_and_replay():
    """The trio tracked coherently through TrackingResult on a DeviceFile at file offset 4096; two of its rows cancelled - the
    cleaned bytes against the cancellation's contract on the GPU's own series, the bar of tests/test_cancel_gpu.py; PRN 22
    tracked coherently on the DeviceFile that cancel() returns, against the contract on its downloaded bytes; and the
    coherent result replayed at the early, prompt and late taps, the bar of tests/test_replay_gpu.py."""
    m = pkg()
    s, rec, chans, edges = _trio()
    off = cases.CANCEL_OFF
    run = cases.CANCEL_RUN
    moved, e2 = cases.moved_behind(chans, edges, off)
    ps = _settings(m, s, trackCoherentMs=run["T"], trackPullInMs=run["P"], trackHandOverMs=run["H"], msToProcess=float(run["ms"]))
    ctx = m.engine.get_context(ps, 0)
    dev = ctx.upload(rec[off:])
    fid = m.DeviceFile(dev, off)
    t = _tracker(m, ps, moved)
    old = type(ctx).track_coherent
    try:
        # (TrackingResult.track finds the edges itself from P = 220 on; here they are given, as the case says)
        type(ctx).track_coherent = lambda self, r, c, ms, p, **kw: old(self, r, c, ms, p, bit_edge=e2[:3], **kw)
        try:
            t.track(fid)
        finally:
            type(ctx).track_coherent = old
        want = spec.track(s, moved, rec, edges=e2, **run)
        pick = {k: v[:3] for k, v in want.items()}
        _same((t.series, np.full(3, run["ms"], dtype=np.int32), t.bitEdge, t.coherentStart, t.edgeEnergy), pick)
        # cancel rows 0 and 1
        cleaned = t.cancel(fid, rows=[0, 1])
        try:
            assert isinstance(cleaned, m.DeviceFile) and cleaned.file_offset == off and len(cleaned.record) == len(dev)
            two, ser = moved[:2], np.ascontiguousarray(t.series[:2])
            amp = cancel_spec.design(ser, cancel_spec.states(s, len(dev), off, two, ser, None))
            ref, v, clipped, covered = cancel_spec.cancel(s, rec[off:], off, two, ser, None, amp)
            y = cleaned.record.download()
            differ = np.flatnonzero(y != ref)
            print("\n[coherent tracking] cancel: %d of %d bytes differ from the contract, all of them ties" % (differ.size, y.size))
            assert np.all(cancel_spec.decisions(v, covered)[differ]) and differ.size <= 1e-4 * y.size and cleaned.clipped == clipped
            assert covered.any() and np.any(y != rec[off:])
            # PRN 22 on the cleaned record
            image = np.r_[np.zeros(off, dtype=np.int8), y]
            want22 = spec.track(s, moved[2:3], image, edges=e2[2:3], **run)
            assert list(want22["ms_done"]) == [run["ms"]]
            got22 = ctx.track_coherent(cleaned.record, moved[2:3], run["ms"], m._native.coh_params(ps), bit_edge=e2[2:3],
                                       rec_file_offset=cleaned.file_offset)
            _same(got22, want22)
        finally:
            cleaned.record.free()
        # the replay of the coherent result
        spacing = float(ps.dllCorrelatorSpacing)
        r = t.replay(fid, [-spacing, 0.0, spacing])
        worst = 0.0
        for c in range(3):
            rms = max(1.0, float(np.sqrt(np.mean(t.series[c, 3] ** 2 + t.series[c, 7] ** 2))))
            for tap, (i_row, q_row) in enumerate(((4, 6), (3, 7), (5, 8))):
                worst = max(worst, float(np.max(np.abs(r.I[c, tap] - t.series[c, i_row]))) / rms,
                            float(np.max(np.abs(r.Q[c, tap] - t.series[c, q_row]))) / rms)
        print("\n[coherent tracking] replay of the early, prompt and late taps: max error %.3g of RMS|P| (bar 1e-6)" % worst)
        assert worst < 1e-6
    finally:
        dev.free()
