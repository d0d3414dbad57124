"""The antenna combiner in the composed contract of tests/chain_cases.py, as far as it runs without a GPU: for every
multi-antenna chain of tests/test_chain_array_gpu.py the package's _walk, _prepared_settings and _file_range against the
contract's maps - a frame of all antennas is one more unit beside a pair, a group of D, a multiple of M and a packed frame -
with the maps of five settings written out; the refusals, which come before anything is opened; the files shown to tell a
wrong combiner from a right one, on the contract alone: no antenna's taps are zero or another's, the combined record clips
a little, and five deliberate mistakes of the composition each change the prepared record; the inputs of the notch and the
monitor chains and the end-to-end scene shown to be well conditioned.  Run with -m "not gpu"."""
import numpy as np
import pytest

import chain_array_scene as scene
import chain_cases as cases
from conftest import pkg
from test_chain_gpu import rounding_count

CHAINS = cases.array_matrix() + list(cases.ARRAY_VARIANTS) + list(cases.ARRAY_NOTCHES)
IDS = [c.name for c in CHAINS]
POSITIONS = CHAINS + [scene.CHAIN]


def test_the_tables_count():
    matrix = cases.array_matrix()
    assert len(matrix) == 24 and len(set(IDS)) == len(CHAINS) == 32
    assert all(c.antennas == 3 and not c.array_block_ms and cases.array_of(c)[1] == (1 if c.iq else 5) for c in matrix)
    assert [c.name for c in matrix[:3]] == ["int8-a3", "int8-a3-r5_3", "int8-a3-iq"]
    assert (cases.ARRAY_BLOCK_REAL.name, cases.ARRAY_BLOCK_IQ.name, cases.ARRAY_HOLD.name, cases.ARRAY_EIGHT.name,
            cases.ARRAY_TWO.name, cases.ARRAY_PACKED_BYTES.name, cases.ARRAY_NOTCH.name, cases.ARRAY_MONITOR.name) == \
        ("int8-a3b-d2-r5_3", "uint8-a3b-iq", "uint8-a3b-d2", "int8-a8k1-iq", "int8-a2k15ref1", "packed2-a3", "int8-a3-d2-notch",
         "uint8-a3-iq-notch")
    for c in (cases.ARRAY_BLOCK_REAL, cases.ARRAY_BLOCK_IQ, cases.ARRAY_HOLD):
        assert cases.array_of(c)[3:] == (cases.ARRAY_BLOCK_FRAMES, 3) == (4096, 3)
    # the chains from before the combiner keep their names
    assert [c.name for c in cases.matrix()[:4]] == ["none", "none-r5_3", "none-iq", "none-iq-r5_3"]
    assert cases.VARIANT_QI_U8.name == "uint8-d4-qi-r3_1" and cases.VARIANT_FRAME.name == "packed2_f4_1-d2"


# ---- the maps, written out ------------------------------------------------------------------------------------------------

def _names(steps):
    return [(stage.name, n_in, n_out) for stage, _, n_in, n_out in steps]


def test_the_maps_written_out():
    m = pkg()
    # a real offset-binary file of three antennas, decimated by 2 and resampled by 5/3
    c = cases.Chain(dtype="uint8", antennas=3, D=2, resamp=(5, 3), fs=16368000.0, f0=2000000.0)
    s = c.settings(m)
    assert _names(s._walk()[0]) == cases.walk(c) == [("combine", 3, 1), ("decimate", 2, 1), ("resample", 3, 5)]
    assert s._prepared_settings().samplingFreq == cases.prepared_settings(c)["samplingFreq"] == 13640000.0
    for (offset, count), want in (((0, 5000), (0, 18000)), ((5, 5001), (18, 18006)), ((10, 77), (36, 282))):
        assert s._file_range(offset, count) == cases.file_range(c, offset, count) == want
    # the same as I/Q, the carrier 1 MHz below the centre
    c = cases.Chain(dtype="uint8", antennas=3, D=2, iq=True, resamp=(5, 3), fs=8184000.0, f0=-1000000.0)
    s = c.settings(m)
    assert _names(s._walk()[0]) == cases.walk(c) == [("combine", 6, 2), ("decimate", 4, 2), ("convert", 2, 2), ("resample", 3, 5)]
    for (offset, count), want in (((0, 5000), (0, 18000)), ((10, 77), (36, 288))):
        assert s._file_range(offset, count) == cases.file_range(c, offset, count) == want
    for refuses in (s._file_range, lambda o, n: cases.file_range(c, o, n)):
        with pytest.raises(ValueError, match="pair"):
            refuses(5, 77)                                                     # sample 3 in front of the resampler: a Q
    # four antennas of I/Q in a packed frame of eight 4-bit fields
    c = cases.Chain(first="packed", bits=4, frame=8, antennas=4, iq=True, fs=cases.IQ_FILE[0], f0=cases.IQ_FILE[1])
    s = c.settings(m)
    assert _names(s._walk()[0]) == cases.walk(c) == [("unpack", 4, 8), ("combine", 8, 2), ("convert", 2, 2)]
    assert s._file_range(2, 5001) == cases.file_range(c, 2, 5001) == (4, 10004)
    # 2-bit samples of three antennas, four to a byte: whole bytes and whole frames of all antennas, 3 bytes
    c = cases.Chain(first="packed", bits=2, frame=1, antennas=3, array_taps=5)
    s = c.settings(m)
    assert _names(s._walk()[0]) == cases.walk(c) == [("unpack", 1, 4), ("combine", 3, 1)]
    assert s._file_range(0, 5000) == cases.file_range(c, 0, 5000) == (0, 3750)
    assert s._file_range(0, 5001) == cases.file_range(c, 0, 5001) == (0, 3753)
    assert s._file_range(4, 5001) == cases.file_range(c, 4, 5001) == (3, 3753)
    # the constants the block grid rests on
    assert m._native.combine_tile() == 4096 and m._native.ARRAY_BLOCK_UNIT == 4096
    s = cases.Chain(antennas=3, array_block_ms=1.0, fs=16368000.0).settings(m)
    assert s._array_block_format() == (16384, 3) and cases.array_of(cases.Chain(antennas=3, array_block_ms=1.0))[3] == 16384


def _packed_frame_one_layouts():
    """Every packedFrame = 1 layout whose samples per byte are not whole frames of all antennas."""
    out = []
    for bits in (1, 2, 4):
        for A in range(2, 9):
            for iq in (False, True):
                if (8 // bits) % (A * (2 if iq else 1)) and A * (1 if iq else 5) <= 64:
                    out.append((bits, A, iq))
    return out


def test_packed_bytes_and_antenna_frames_round_to_their_common_multiple():
    """1-bit with 3, 5, 6, 7 antennas, 2-bit with 3, 5, 6, 7, 8, 4-bit with 3 .. 8, real and I/Q: for every count of three
    such runs _file_range gives whole bytes that are whole frames of all antennas, the least that hold the count."""
    m = pkg()
    layouts = _packed_frame_one_layouts()
    assert (1, 3, False) in layouts and (2, 8, False) in layouts and (2, 3, True) in layouts and (1, 8, False) not in layouts
    for bits, A, iq in layouts:
        c = cases.Chain(first="packed", bits=bits, frame=1, antennas=A, iq=iq, fs=cases.IQ_FILE[0], f0=cases.IQ_FILE[1])
        s = c.settings(m)
        frame, per_byte = A * c.lanes, 8 // bits
        whole = int(np.lcm(frame, per_byte))
        for count in range(c.lanes, 3 * whole // A + 2, c.lanes):
            first, n_bytes = s._file_range(0, count)
            assert (first, n_bytes) == cases.file_range(c, 0, count), (c.name, count)
            samples = n_bytes * per_byte
            assert samples % frame == 0 and samples % whole == 0 and 0 <= samples - count * A < whole, (c.name, count)


# ---- the maps of every chain ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chain", POSITIONS, ids=[c.name for c in POSITIONS])
def test_walk_and_prepared_settings(chain):
    m = pkg()
    s = chain.settings(m)
    steps, real = s._walk()
    assert _names(steps) == cases.walk(chain), chain.name
    assert ("combine", chain.antennas * chain.lanes, chain.lanes) in cases.walk(chain)
    want = cases.prepared_settings(chain)
    assert dict((k, getattr(real, k)) for k in want) == want, chain.name
    assert not (real.antennas or real.iqRecord or real.decimation or real.resampleUp or real.packedBits)
    assert s.antennas == chain.antennas and s.dataType == chain.dtype and s.samplingFreq == chain.fs     # left alone


@pytest.mark.parametrize("chain", POSITIONS, ids=[c.name for c in POSITIONS])
def test_skip_mapping(chain):
    """Every skipNumberOfBytes up to two units and one byte, and one far out: the legal ones - the multiples of the
    contract's unit - map to the contract's sample, the others are refused with the setting's name, the byte inside a frame
    of all antennas among them; and _file_range undoes the map."""
    m = pkg()
    unit = cases.skip_unit(chain)
    frame_bytes = chain.antennas * chain.lanes * (chain.bits if chain.first == "packed" else 8)
    if chain.first == "packed" and chain.frame > 1:
        frame_bytes = chain.frame * chain.bits
    assert (8 * unit) % frame_bytes == 0, chain.name                           # whole frames of all antennas
    legal = []
    tried = list(range(0, 2 * unit + 2)) + [1237 * unit, 1237 * unit + 1]
    for skip in tried:
        s = chain.settings(m, skipNumberOfBytes=skip)
        try:
            want = cases.prepared_skip(chain, skip)
        except ValueError:
            with pytest.raises(ValueError, match="skipNumberOfBytes"):
                s._prepared_settings()
            with pytest.raises(ValueError, match="skipNumberOfBytes"):
                with s._prepared_record("/nonexistent/record.bin", 0, 1000):
                    pass
            continue
        legal.append(skip)
        assert s._prepared_settings().skipNumberOfBytes == want, (chain.name, skip)
        assert s._file_range(want, chain.lanes)[0] == skip, (chain.name, skip)
    assert legal == [skip for skip in tried if skip % unit == 0], (chain.name, unit, legal)
    if frame_bytes > 8:
        with pytest.raises(ValueError, match="a frame of all antennas|a frame of the packed file"):
            chain.settings(m, skipNumberOfBytes=frame_bytes // 8 - 1)._prepared_settings()
    step = cases.prepared_skip(chain, unit)
    assert step == cases.smallest_offset(chain) and cases.prepared_skip(chain, 2 * unit) == 2 * step


@pytest.mark.parametrize("chain", POSITIONS, ids=[c.name for c in POSITIONS])
def test_file_range(chain):
    """Settings._file_range(offset, count) is the contract's file_range() - or both refuse, _prepared_record with a path
    that does not exist too - for offset 0, every offset below two legal steps and one byte, one far out, and counts that
    need every rounding: a multiple of everything, one more, and the odd and even counts around a step."""
    m = pkg()
    s = chain.settings(m)
    step = cases.smallest_offset(chain)
    whole = step * 12 * 1000
    legal = refused = 0
    for offset in list(range(0, 2 * step + 2)) + [1237 * step, 1237 * step + 1]:
        for count in (whole, whole + 1, whole + 2, 1000, 1001, step + 1, step + 2):
            try:
                want = cases.file_range(chain, offset, count)
            except ValueError:
                refused += 1
                with pytest.raises(ValueError):
                    s._file_range(offset, count)
                with pytest.raises(ValueError):
                    with s._prepared_record("/nonexistent/record.bin", offset, count):
                        pass
                continue
            legal += 1
            assert s._file_range(offset, count) == want, (chain.name, offset, count)
            assert want[0] % (chain.antennas * chain.lanes) == 0 or chain.first == "packed", (chain.name, offset)
    assert legal >= 21 and (refused > 0 or step == 1), chain.name
    assert cases.file_range(chain, 0, whole)[1] < cases.file_range(chain, 0, whole + 1)[1] or chain.iq, chain.name


# ---- refusals, before anything is opened --------------------------------------------------------------------------------------

def _refused(chain, match, **kw):
    s = chain.settings(pkg(), **kw)
    with pytest.raises(ValueError, match=match):
        s._prepared_settings()
    with pytest.raises(ValueError, match=match):
        with s._prepared_record("/nonexistent/record.bin", 0, 1000):
            pass
    if not kw:
        with pytest.raises(ValueError):
            cases.prepared_settings(chain)


def test_refusals_come_before_the_file():
    fs, f0 = cases.IQ_FILE
    _refused(cases.Chain(first="cond", antennas=3), "frontEndConditioning")
    _refused(cases.Chain(first="cond", dtype="int16", antennas=3, iq=True, fs=fs, f0=f0), "frontEndConditioning")
    _refused(cases.Chain(first="requant", dtype="int16", antennas=3, iq=True, fs=fs, f0=f0), "iqRequantize")
    _refused(cases.Chain(first="requant", dtype="float32", antennas=3, iq=True, fs=fs, f0=f0), "iqRequantize")
    for dtype in ("int16", "float32"):
        _refused(cases.Chain(dtype=dtype, antennas=3), "out of scope")
        _refused(cases.Chain(dtype=dtype, antennas=3, iq=True, D=2, fs=cases.IQ_FILE_DECIMATED[0], f0=cases.IQ_FILE_DECIMATED[1]),
                 "out of scope")
    _refused(cases.Chain(antennas=5, array_taps=13), "more than 64 weights")
    _refused(cases.Chain(antennas=8, array_taps=9, resamp=(5, 3)), "more than 64 weights")
    _refused(cases.Chain(antennas=9), "antennas")
    _refused(cases.Chain(antennas=3, array_reference=3), "arrayReference")
    _refused(cases.Chain(first="packed", bits=2, frame=4, antennas=3, first_field=2), "packedFirst")
    for chain in (cases.array_chain("none", "int8", True, False, True), cases.array_chain("none", "uint8", False, True, False),
                  cases.ARRAY_EIGHT):
        frame = chain.antennas * chain.lanes
        for skip in (1, frame - 1, frame + 1):
            _refused(chain, "skipNumberOfBytes = %d splits a frame of all antennas" % skip, skipNumberOfBytes=skip)
            with pytest.raises(ValueError, match="a frame of all antennas"):
                cases.prepared_skip(chain, skip)


# ---- the inputs discriminate ----------------------------------------------------------------------------------------------

_FILES = {}


def _file(chain):
    if chain.name not in _FILES:
        b = cases.array_file_of(chain, pkg()._native)
        b.setflags(write=False)
        _FILES[chain.name] = b
    return _FILES[chain.name]


def _probe(chain, total):
    """The offset and count of run_chain's probe beyond the first tile seam: the window the GPU test compares in."""
    native = pkg()._native
    step = cases.smallest_offset(chain)
    offset = (cases.largest_tile(chain, native) // step + 3) * step
    return offset, rounding_count(chain, total - offset - 2 * step - 2 * cases.rounding_unit(chain))


def _tap_sets(taps, chain):
    """[blocks or 1][A] of the taps as bytes."""
    t = np.asarray(taps)
    if not chain.array_block_ms:
        t = t[None]
    return [[t[j, a].tobytes() for a in range(chain.antennas)] for j in range(t.shape[0])]


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_the_files_tell_a_wrong_combiner_from_a_right_one(chain):
    b = _file(chain)
    assert b.size < 1 << 20 and np.unique(b[:256]).size == 256
    total = cases.prepared_length(chain, b.size)
    assert total >= cases.prepared_size(chain, pkg()._native)
    A, K, ref, B, W = cases.array_of(chain)
    offset, count = _probe(chain, total)
    first = cases.file_range(chain, offset, count)[0]
    for at, n in ((0, total), (offset, count)):
        true = cases.prepare(b, chain, at, n)
        c = true["combine"]
        sets = _tap_sets(c["taps"], chain)
        for j, block in enumerate(sets):
            if B and c["status"][j]:
                continue
            assert all(np.frombuffer(t, dtype=np.int16).any() for t in block), (chain.name, at, j)      # no antenna is left out
            assert len(set(block)) == A, (chain.name, at, j)                                        # and none is another
        print("%s at %d: %d of %d samples clipped (%.4f %%), arrayTargetRms %g" %
              (chain.name, at, c["clipped"], c["samples"], 100.0 * c["clipped"] / c["samples"], chain.array_target_rms))
        assert 0 < c["clipped"] < 0.01 * c["samples"], (chain.name, at, c["clipped"], c["samples"])
        if B:
            assert c["blocks"] == -(-c["samples"] // chain.lanes // B) >= 10 and c["block_frames"] == B == 4096
            assert len(set(b"".join(block) for block in sets)) > c["blocks"] // 2, chain.name      # the weights follow the file
    if B:                                                                      # the probe starts off the grid of blocks
        assert first % (A * chain.lanes) == 0 and (first // (A * chain.lanes)) % B, (chain.name, first)
        whole = cases.prepare(b, chain, 0, total)["combine"]
        assert whole["held"] == (cases.ARRAY_HOLD_HELD if chain is cases.ARRAY_HOLD else 0), (chain.name, whole["held"])
        if chain is cases.ARRAY_HOLD:
            j0, j1 = cases.ARRAY_ZERO_BLOCKS[chain.name]
            assert j1 - j0 >= W + 1 and list(np.flatnonzero(whole["status"])) == list(range(j0 + 1, j1 - 1))
            x = (b ^ 0x80).view(np.int8).reshape(-1, A)
            assert not x[j0 * B:j1 * B].any() and x[j0 * B - 1].any() and x[j1 * B].any()
            assert true["combine"]["held"] > 0                                 # behind the offset the rule still runs
    # the deliberate mistakes: each changes the prepared record inside the compared window
    flaws = ["file_stats"]
    if A >= 3:
        flaws.append("swap")
    if B:
        flaws.append("grid")
    if chain.dtype == "uint8" and (chain.D or chain.iq):
        flaws.append("offset_binary")
    if chain.first == "packed" and chain.frame > 1:
        flaws.append("first_field")
    y = true["record"]
    for flaw in flaws:
        wrong = cases.prepare(b, chain, offset, count, flaw=flaw)["record"]
        differ = int(np.count_nonzero(wrong[:y.size] != y[:wrong.size])) if wrong.size == y.size else -1
        print("%s, %s: %d of %d bytes differ" % (chain.name, flaw, differ, y.size))
        assert wrong.size == y.size and differ > 0, (chain.name, flaw)


def test_every_flaw_is_tried_somewhere():
    seen = set()
    for chain in CHAINS:
        seen.add("file_stats")
        seen.update(["swap"] if chain.antennas >= 3 else [])
        seen.update(["grid"] if chain.array_block_ms else [])
        seen.update(["offset_binary"] if chain.dtype == "uint8" and (chain.D or chain.iq) else [])
        seen.update(["first_field"] if chain.first == "packed" and chain.frame > 1 else [])
    assert seen == set(cases.FLAWS)


# ---- the inputs of the notch and of the monitor ---------------------------------------------------------------------------

def test_the_line_survives_the_combiner():
    """The files of the two chains that end in the notch, through the composed contract: one line, where the file put it,
    and no bin within 1 dB of notchThresholdDb - in the oracle's spectrum of ten code periods and in the monitor's max-hold."""
    m = pkg()
    for chain in cases.ARRAY_NOTCHES:
        s = chain.settings(m, **(cases.ARRAY_MONITOR_SETTINGS if chain is cases.ARRAY_MONITOR else {}))
        b = _file(chain)
        composed = cases.prepare(b, chain, 0, cases.prepared_length(chain, b.size))
        at = cases.smallest_offset(chain)
        if chain is cases.ARRAY_MONITOR:
            w, lines, taps = cases.monitor_contract(chain, composed, at, s.notchThresholdDb, s.notchWidthHz, s.notchTaps,
                                                    s.monitorSliceMs, s.monitorSegment, s.monitorOverlap)
            assert w["pxx"].shape[0] >= 4 and int(w["n_segments"].min()) >= 6
        else:
            lines, taps = cases.notch_contract(chain, composed, at, s.notchThresholdDb, s.notchWidthHz, s.notchTaps)
        assert len(lines) == 1 and taps.size == s.notchTaps
        assert cases.ARRAY_LINE_AMPLITUDE < cases.ARRAY_NOISE                  # under the noise of every antenna


# ---- the scene ----------------------------------------------------------------------------------------------------------------

def test_the_scene_is_well_conditioned():
    """The composed contract's record of the scene under the oracle's search, in both windows the GPU test acquires in:
    the scene's four satellites, each at least MARGIN above the threshold, every absent PRN at or below ABSENT_MAX; the
    C/A band below the resampler's cutoff; the skip whole frames of all antennas and a whole group of M."""
    m = pkg()
    chain = scene.CHAIN
    r = cases.rates(chain)                                                     # (refuses a band the low-pass cuts into)
    assert (r["fs"], r["IF"]) == (13640000.0, 2046000.0) and r["resamp"] is not None
    assert r["IF"] + cases.CHIP_RATE < cases.resamp_spec.default_cutoff(2.0 * chain.fs, *chain.resamp)
    o = scene.oracle_settings()
    real = scene.settings(m)._prepared_settings()
    assert (real.samplingFreq, real.IF, real.samplesPerCode) == (o.samplingFreq, o.IF, o.samplesPerCode)
    frame = chain.antennas * chain.lanes
    assert scene.SKIP_BYTES % frame == 0 and (scene.SKIP_BYTES // frame * chain.lanes) % chain.resamp[1] == 0
    absent = [p for p in range(1, 33) if p not in scene.PRNS]
    assert len(absent) == 28 and len(scene.PRNS) == 4
    for skip in (0, scene.SKIP_BYTES):
        assert scene.settings(m, skipNumberOfBytes=skip)._prepared_settings().skipNumberOfBytes == cases.prepared_skip(chain, skip)
        assert scene.need(skip) <= cases.prepared_length(chain, scene.file_bytes().size)
        ref = scene.contract_acquisition(skip)
        pm = np.asarray(ref["peakMetric"])
        print("skip %d: peak metrics %s, largest among the 28 absent PRNs %.3f"
              % (skip, np.round(pm[[p - 1 for p in scene.PRNS]], 2), float(pm[[p - 1 for p in absent]].max())))
        assert sorted(np.flatnonzero(ref["carrFreq"]) + 1) == sorted(scene.PRNS)
        assert pm[[p - 1 for p in scene.PRNS]].min() >= scene.MARGIN * o.acqThreshold
        assert pm[[p - 1 for p in absent]].max() <= scene.ABSENT_MAX
