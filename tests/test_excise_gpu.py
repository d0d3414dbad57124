"""Swept-interference excision on the GPU (sgx_if_excise, csrc/sgx_excise.hip; Settings.sweptMitigation): the kernel against
the host run of the same work items (sgx_excise_host) and against the numpy contract of tests/excise_spec.py, byte for byte,
on every case of tests/excise_cases.py; then the stage inside the prepared record, composed with its neighbours, and on a
record beyond 4 GiB.  Run with -m gpu."""
import numpy as np
import pytest

import excise_cases as cases
import excise_spec as spec
from conftest import pkg

pytestmark = pytest.mark.gpu

FIGURES = ("segments", "bins_cut", "segments_cut", "clipped")


@pytest.fixture(scope="module")
def ctx():
    m = pkg()
    return m.engine.get_context(m.Settings(), 0)


def run(ctx, x, N=256, threshold=8.0, passes=3):
    rec = ctx.upload(x)
    try:
        out, info = ctx.excise_record(rec, N, threshold, passes)
        try:
            assert len(out) == x.size
            return out.download(), info
        finally:
            out.free()
    finally:
        rec.free()


def same(got, want, what):
    (y, info), (y0, info0) = got, want
    assert y.dtype == np.int8 and y.size == y0.size
    assert y.tobytes() == y0.tobytes(), "%s: first difference at sample %d" % (what, int(np.flatnonzero(y != y0)[0]))
    assert [info[k] for k in FIGURES] == [info0[k] for k in FIGURES], what
    assert np.array_equal(info["cut_per_segment"], info0["cut_per_segment"]), what


@pytest.mark.parametrize("c", cases.CASES, ids=[c.name for c in cases.CASES])
def test_the_kernel_equals_the_host_items_and_the_contract(ctx, c):
    got = run(ctx, c.x, c.N, c.threshold, c.passes)
    same(got, pkg()._native.excise_host(c.x, c.N, c.threshold, c.passes), "host items")
    same(got, c.reference(), "contract")


def test_two_calls_give_the_same_bytes_and_leave_the_input_alone(ctx):
    c = cases.BY_NAME["chirp_noise_N256"]
    rec = ctx.upload(c.x)
    try:
        a, ia = ctx.excise_record(rec, c.N, c.threshold, c.passes)
        b, ib = ctx.excise_record(rec, c.N, c.threshold, c.passes)
        ga, gb = a.download(), b.download()
        a.free()
        b.free()
        assert rec.download().tobytes() == c.x.tobytes()
    finally:
        rec.free()
    same((ga, ia), (gb, ib), "second call")
    assert ctx.excise_timing() > 0.0


def test_timing_is_zero_with_no_work():
    m = pkg()
    with m.engine.private_context(m.Settings(), 0) as c:      # a context that has not run the stage
        assert c.excise_timing() == 0.0
        rec = c.upload(cases.BY_NAME["noise_N64"].x)
        try:
            out, _ = c.excise_record(rec, 64)
            out.free()
            assert c.excise_timing() > 0.0
            with pytest.raises(m._native.SgxError):           # a refusal launches nothing
                c.excise_record(rec, 96)
        finally:
            rec.free()


# ---- the stage inside the prepared record ---------------------------------------------------------------------------------

def _acquire(m, s, rec):
    n = s.samplesPerCode
    a = m.AcquisitionResult(s, device=0)
    a.acquire(m.DeviceSignal(rec, 0, 11 * n))
    return a


def test_the_chirp_scene_through_swept_mitigation(tmp_path):
    """Settings.sweptMitigation: the prepared record is the contract's excised record, and its acquisition is, exactly, the
    acquisition of those bytes uploaded as a plain record - all eight satellites; with the stage off the prepared record is
    the raw one, which loses them."""
    import chirp_scene
    m = pkg()
    x = chirp_scene.record()
    want, want_info = chirp_scene.excised()
    path = str(tmp_path / "chirp.bin")
    x.tofile(path)
    s = m.Settings()
    with s._prepared_record(path, 0, x.size) as rec:               # the stage is off: the raw record
        assert rec.download().tobytes() == x.tobytes()
        raw = _acquire(m, s, rec)
    assert not hasattr(s, "lastExcision")
    s.sweptMitigation = True
    with s._prepared_record(path, 0, x.size, mitigate_at=0) as rec:
        assert rec.download().tobytes() == want.tobytes()
        got = _acquire(m, s, rec)
    info = s.lastExcision
    assert [info[k] for k in FIGURES] == [want_info[k] for k in FIGURES]
    assert np.array_equal(info["cut_per_segment"], want_info["cut_per_segment"])
    assert info["cells_cut"] == want_info["bins_cut"] / float(want_info["segments"] * 127)
    assert not hasattr(s, "lastNotchLines")                         # the notch was not asked for
    plain = m.engine.get_context(s, 0).upload(want)
    try:
        ref = _acquire(m, s, plain)
    finally:
        plain.free()
    for k in ("carrFreq", "codePhase", "peakMetric"):
        assert np.array_equal(getattr(got, k), getattr(ref, k)), k
    assert sorted(np.flatnonzero(got.carrFreq) + 1) == list(chirp_scene.PRNS)
    assert np.count_nonzero(raw.carrFreq[chirp_scene.PRN_INDICES]) <= len(chirp_scene.PRNS) // 2
    oracle = chirp_scene.search("excised")
    assert np.array_equal(got.codePhase[chirp_scene.PRN_INDICES], oracle["codePhase"][chirp_scene.PRN_INDICES])


def test_behind_the_converter_and_in_front_of_the_notch(tmp_path):
    """An interleaved I/Q file with a line through the converter, the excision (threshold 5: 1.2 % of the cells go) and the
    notch, against the contracts chained: chain_cases.prepare, excise_spec.excise, then the notch designed from the oracle's
    spectrum of the EXCISED record (chain_cases.notch_contract holds it clear of the threshold by 1 dB) and applied to it."""
    import chain_cases
    import notch_spec
    m = pkg()
    chain = chain_cases.matrix_chain("none", "int8", False, True, False)
    s = chain.settings(m, interferenceMitigation=True, sweptMitigation=True, exciseThreshold=5.0)
    b = chain_cases.line_file(chain, np.random.default_rng(chain_cases.LINE_SEED),
                              chain_cases.file_components(chain, chain_cases.prepared_size(chain, m._native)))
    path = str(tmp_path / "iq_line.bin")
    b.tofile(path)
    total = chain_cases.prepared_length(chain, b.size)
    at = chain_cases.smallest_offset(chain)
    composed = chain_cases.prepare(b, chain, 0, total)
    y, info = spec.excise(composed["record"], 256, 5.0, 3, margins=True)
    assert min(info["margin_compare"], info["margin_round"]) >= spec.MARGIN and info["bins_cut"] > 500
    lines, taps = chain_cases.notch_contract(chain, dict(composed, record=y), at, s.notchThresholdDb, s.notchWidthHz,
                                             s.notchTaps)
    want = notch_spec.apply(y, taps, notch_spec.DESIGN_SHIFT)
    assert np.count_nonzero(want != y) > y.size // 2
    with s._prepared_record(path, 0, total, mitigate_at=at) as rec:
        got = rec.download()
    assert s.lastNotchLines == lines
    assert [s.lastExcision[k] for k in FIGURES] == [info[k] for k in FIGURES]
    assert got.tobytes() == want.tobytes(), "first difference at sample %d" % int(np.flatnonzero(got != want)[0])


# ---- a record beyond 4 GiB --------------------------------------------------------------------------------------------------

BIG_N, BIG_THRESHOLD, BIG_WINDOW = 256, 3.0, 8192


def test_a_record_beyond_4_gib():
    """The default scene, 2^32 + 100 code periods made on the device, through the stage at threshold 3 (5 % of the cells
    go, so every window is rebuilt samples): windows at both ends, around sample 2^31 and around 2^32, each against the
    contract run on that window alone - which starts on a hop, so its segments are the record's - without the N samples at
    the window's own edges.  tests/big_record.py's rule first: positions reduced by 2^32 or 2^31 give other bytes."""
    import big_record as big
    m = pkg()
    ctx = m.engine.get_context(m.Settings(), 0)
    sc = m.synth.Scene.default()
    at = big.scene_reader(m.synth.generate, sc)
    n, N, H, W = big.SCENE_N, BIG_N, BIG_N // 2, BIG_WINDOW
    windows = [(0, W), (big.B32 // 2 - W // 2, big.B32 // 2 + W // 2), (big.B32 - W // 2, big.B32 + W // 2),
               ((n - W) // H * H, n)]
    per_window = {}

    def contract(read, w0, w1):
        y, info = spec.excise(read(w0, w1), N, BIG_THRESHOLD, 3, margins=True)
        assert min(info["margin_compare"], info["margin_round"]) >= spec.MARGIN, (w0, info)
        if read is at:
            per_window[w0] = info["cut_per_segment"]
        return y[(N if w0 else 0):y.size - (N if w1 < n else 0)]

    # (in front of the record both wrapped readings find nothing: the rule has no hold on the first window)
    wants = [(w, big.wrap_visible(at, contract, w) if w[0] else contract(at, *w)) for w in windows]
    dev = ctx.synth(sc, n)
    try:
        out, info = ctx.excise_record(dev, N, BIG_THRESHOLD, 3)
        try:
            assert len(out) == n and info["segments"] == spec.segments(n, N) == info["cut_per_segment"].size
            for (w0, w1), want in wants:
                lo, hi = w0 + (N if w0 else 0), w1 - (N if w1 < n else 0)
                got = out.download(lo, hi - lo)
                assert got.tobytes() == want.tobytes(), \
                    "window [%d, %d) differs first at sample %d" % (w0, w1, lo + int(np.flatnonzero(got != want)[0]))
                per = per_window[w0]                   # the segments that lie inside the window whole (or past the record's ends)
                first, last = (1 if w0 else 0), (per.size - 2 if w1 < n else per.size - 1)
                assert np.array_equal(info["cut_per_segment"][w0 // H + first:w0 // H + last + 1], per[first:last + 1]), w0
                assert per[first:last + 1].sum() > 0
            assert 0.01 < info["bins_cut"] / float(info["segments"] * (H - 1)) < 0.2
        finally:
            out.free()
    finally:
        dev.free()
