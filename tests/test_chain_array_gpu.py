"""The antenna combiner composed with every stage around it, on the GPU: Settings._prepared_record for the multi-antenna
chains of tests/chain_cases.py (array_matrix(): first stage x decimation x iqRecord x resampleUp at three antennas; the
variants: weights per block, a stretch of zeros that the hold rule bridges, eight antennas, two antennas with 15 taps and
the second as the reference, a packed file whose bytes are not whole frames of all antennas) against the composed contract,
byte for byte, through the five probes of tests/test_chain_gpu.py's run_chain - the whole file, the smallest legal offset,
an offset beyond the first tile seam with a count that needs every rounding, an odd count, a file that ends early - with
every stage's counts, lastCombining among them; a chain that ends in the notch and one in the whole-record monitor; then the
I/Q scene of tests/array_cases.py with a 5/3 resampler behind the converter, end to end.  Run with -m gpu."""
import subprocess
import sys

import numpy as np
import pytest

import chain_array_scene as scene
import chain_cases as cases
import notch_spec
from conftest import ROOT, pkg
from oracle import softgnss_oracle as orc
from record_stage import same_tracking
from test_array_gpu import _same_search
from test_chain_gpu import check_counts, largest_tile, prepared, run_chain, same_bytes, step_of
from test_gpu_parity import PSD_TOL
from test_waterfall_gpu import spectrum_error

pytestmark = pytest.mark.gpu

MATRIX = cases.array_matrix()


def run_array_chain(tmp_path, chain):
    """run_chain, whose file of a multi-antenna chain is chain_cases.array_file()'s - the one tests/test_chain_array_host.py
    has shown to tell a wrong combiner from a right one."""
    run_chain(tmp_path, chain)
    b = np.fromfile(str(tmp_path / (chain.name + ".bin")), dtype=np.uint8)
    assert b.tobytes() == cases.array_file_of(chain, pkg()._native).tobytes()
    return b


@pytest.mark.parametrize("chain", MATRIX, ids=[c.name for c in MATRIX])
def test_array_chain(tmp_path, chain):
    run_array_chain(tmp_path, chain)


@pytest.mark.parametrize("chain", cases.ARRAY_VARIANTS, ids=[c.name for c in cases.ARRAY_VARIANTS])
def test_array_variant(tmp_path, chain):
    """Weights per block behind an offset that is off the grid of blocks - the blocks count from the slice's first frame -
    real in front of the decimator and the resampler and offset binary in front of the converter; the same with a stretch
    of zeros, whose blocks hold a neighbour's weights; eight antennas of I/Q in 16-byte frames; two antennas of 15 taps,
    the second held at 1; 2-bit samples of three antennas, four to a byte, where a count of samples is whole bytes and
    whole frames of all antennas only every 12."""
    A, K, ref, B, W = cases.array_of(chain)
    if B:
        offset = (largest_tile(chain) // step_of(chain) + 3) * step_of(chain)
        first = cases.file_range(chain, offset, 2)[0]
        assert first % (A * chain.lanes) == 0 and (first // (A * chain.lanes)) % B, chain.name
    if chain is cases.ARRAY_PACKED_BYTES:
        assert cases.components_per_unit(chain) == (4, 3) and cases.rounding_unit(chain) == 3
    b = run_array_chain(tmp_path, chain)
    if chain is cases.ARRAY_HOLD:                                              # the whole file once more: what it was built for
        s = chain.settings(pkg())
        want = prepared(s, chain, str(tmp_path / (chain.name + ".bin")), b, 0, cases.prepared_length(chain, b.size))
        assert s.lastCombining["held_blocks"] == want["combine"]["held"] == cases.ARRAY_HOLD_HELD


def test_a_packed_file_of_three_antennas_at_any_count(tmp_path):
    """packedFrame = 1, 2-bit, three antennas: a byte holds four samples, a frame of all antennas three.  Every count of a
    run of twelve - those that are no whole bytes, those that are whole bytes and no whole frames - and a file that ends
    inside a frame of all antennas give the contract's record; the upload is rounded to 3 bytes, 4 frames."""
    chain = cases.ARRAY_PACKED_BYTES
    s = chain.settings(pkg())
    b = cases.array_file_of(chain, pkg()._native)[:3 * 3000]
    path = str(tmp_path / "bytes.bin")
    b.tofile(path)
    assert s._file_range(0, 5000) == (0, 3750) and s._file_range(0, 5001) == (0, 3753)
    for count in range(5000, 5013):
        want = prepared(s, chain, path, b, 8, count)
        assert want["record"].size == -(-count // 4) * 4 and want["file_range"] == (6, want["record"].size // 4 * 3)
    for end in (b.size - 1, b.size - 2, b.size - 3):                          # the file ends inside a frame: the frame is left
        short = path + ".%d" % end
        b[:end].tofile(short)
        want = prepared(s, chain, short, b[:end], 8, 12000, exact=False)
        assert want["file_range"] == (6, b.size - 9) and want["record"].size == 4 * (b.size - 9) // 3


# ---- the notch and the monitor behind the combiner ---------------------------------------------------------------------------

def test_array_chain_into_the_notch(tmp_path):
    """test_chain_gpu.py's test_chain_into_the_notch with the combiner in the chain: the lines the contract finds in the
    oracle's spectrum of the composed record, the contract's filter of them, the composed record through it."""
    chain = cases.ARRAY_NOTCH
    m = pkg()
    s = chain.settings(m, interferenceMitigation=True)
    b = cases.array_file_of(chain, m._native)
    path = str(tmp_path / (chain.name + ".bin"))
    b.tofile(path)
    total = cases.prepared_length(chain, b.size)
    at = step_of(chain)
    with s._prepared_record(path, 0, total, mitigate_at=at) as rec:
        got = rec.download()
    found = s.lastNotchLines
    composed = cases.prepare(b, chain, 0, total)
    check_counts(s, chain, composed, (chain.name, "notch"))
    lines, taps = cases.notch_contract(chain, composed, at, s.notchThresholdDb, s.notchWidthHz, s.notchTaps)
    assert found == lines, (chain.name, found, lines)
    same_bytes(got, notch_spec.apply(composed["record"], taps, notch_spec.DESIGN_SHIFT), (chain.name, "notch"))


def test_array_chain_into_the_whole_record_monitor(tmp_path):
    """notchWholeRecord behind the combiner: the monitor's max-hold spectrum of the composed record from sample `at` on is
    the contract's (tests/waterfall_spec.py) to PSD_TOL as tests/test_waterfall_gpu.py takes it, the lines are those the
    contract finds in its own - no bin within 1 dB of the threshold - and the record is the composed one through the
    contract's filter of them."""
    chain = cases.ARRAY_MONITOR
    m = pkg()
    s = chain.settings(m, interferenceMitigation=True, **cases.ARRAY_MONITOR_SETTINGS)
    b = cases.array_file_of(chain, m._native)
    path = str(tmp_path / (chain.name + ".bin"))
    b.tofile(path)
    total = cases.prepared_length(chain, b.size)
    at = step_of(chain)
    with s._prepared_record(path, 0, total, mitigate_at=at) as rec:
        got = rec.download()
    found, seen = s.lastNotchLines, s.lastMonitor["waterfall"]
    composed = cases.prepare(b, chain, 0, total)
    check_counts(s, chain, composed, (chain.name, "monitor"))
    w, lines, taps = cases.monitor_contract(chain, composed, at, s.notchThresholdDb, s.notchWidthHz, s.notchTaps,
                                            s.monitorSliceMs, s.monitorSegment, s.monitorOverlap)
    assert seen.pxx.shape == w["pxx"].shape and w["pxx"].shape[0] >= 4
    assert np.array_equal(seen.f, w["f"]) and np.array_equal(seen.hist, w["hist"]) and np.array_equal(seen.moments, w["moments"])
    assert max(spectrum_error(seen.pxx, w["pxx"]), spectrum_error(seen.hold, w["hold"])) < PSD_TOL
    assert found == lines, (chain.name, found, lines)
    same_bytes(got, notch_spec.apply(composed["record"], taps, notch_spec.DESIGN_SHIFT), (chain.name, "monitor"))
    events = s.lastMonitor["events"]
    assert len(events) == 1 and abs(events[0][0] - lines[0][0]) <= s.notchWidthHz


# ---- one scene end to end ---------------------------------------------------------------------------------------------------

TRK_MS = scene.TRK_MS


@pytest.fixture(scope="module")
def scene_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("chain_array") / "scene.bin")
    scene.file_bytes().tofile(path)
    return path


@pytest.mark.parametrize("skipped", [False, True], ids=["start", "skip"])
def test_post_processing_of_the_resampled_multi_antenna_scene(scene_path, skipped):
    m = pkg()
    chain = scene.CHAIN
    b = scene.file_bytes()
    skip_bytes = scene.SKIP_BYTES if skipped else 0
    p = cases.prepared_settings(chain, skip_bytes)
    skip, n = p["skipNumberOfBytes"], p["samplesPerCode"]
    s = scene.settings(m, msToProcess=float(TRK_MS), skipNumberOfBytes=skip_bytes)
    acq, trk, nav = s.postProcessing(scene_path)
    assert nav is None or nav._solutions is None
    assert s.skipNumberOfBytes == skip_bytes and s.antennas == chain.antennas and s.resampleUp == chain.resamp[0]    # left alone
    assert dict((k, getattr(acq.settings, k)) for k in p) == p
    assert not (acq.settings.antennas or acq.settings.iqRecord or acq.settings.resampleUp)
    # what the run prepared is the composed contract's record of the bytes it read, with every stage's counts
    count = s.lastResampling["samples"]
    assert skip + TRK_MS * n < count <= cases.prepared_length(chain, b.size)
    want = scene.prepared(scene.need(skip_bytes))                              # (what tests/test_chain_array_host.py looked at)
    assert want["record"].size == count
    check_counts(s, chain, want, ("scene", "postProcessing"))
    with s._prepared_record(scene_path, 0, count) as rec:
        got = rec.download()
    same_bytes(got, want["record"], ("scene", skip_bytes))
    check_counts(s, chain, want, ("scene", "_prepared_record"))
    # acquisition and tracking against the oracle on those bytes
    y = want["record"]
    o = scene.oracle_settings(msToProcess=float(TRK_MS), skipNumberOfBytes=skip)
    ref = orc.acquire(o, y[skip:skip + 11 * n])
    _same_search(acq, ref)
    assert sorted(np.flatnonzero(acq.carrFreq) + 1) == sorted(scene.PRNS)
    chans = orc.pre_run(o, ref)
    assert np.array_equal(acq.channels.PRN, chans["PRN"]) and np.count_nonzero(acq.channels.PRN) == len(scene.PRNS)
    same_tracking(trk, orc.stack_series(orc.track(o, chans, y)), len(scene.PRNS), TRK_MS)


def test_the_resampled_multi_antenna_scene_through_main(scene_path):
    """The command line once: --antennas 4 --iq --resample 5/3 behind a skip, in a process of its own."""
    c = scene.CHAIN
    args = [scene_path, "--fs", repr(c.fs), "--IF", repr(c.f0), "--ms", str(TRK_MS), "--channels", str(len(scene.PRNS)),
            "--skip", str(scene.SKIP_BYTES), "--antennas", str(c.antennas), "--iq", "--resample", "%d/%d" % c.resamp]
    r = subprocess.run([sys.executable, "-m", "softgnss-python_amd.main"] + args, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-2000:]
    assert "Combining %d antennas" % c.antennas in text and "Resampled by %d/%d" % c.resamp in text, text[-2000:]
    assert "Tracking is over" in text, text[-2000:]
