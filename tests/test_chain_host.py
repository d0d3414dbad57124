"""The code that joins the record stages, as far as it runs without a GPU (Settings._prepared_settings, Settings._file_range
and the refusals of Settings._prepared_record, which come before anything is uploaded), against the composed contract of
tests/chain_cases.py:
which chains of stages are accepted - the table is written out below - what rate, IF, sample type and skip each prepared
record is read under, and which skipNumberOfBytes and offsets a chain refuses; the inputs of the notch tests and the two
end-to-end scenes of tests/chain_scenes.py shown to be well conditioned by the contracts and the oracle alone.  Run with
-m "not gpu"."""
import numpy as np
import pytest

import chain_cases as cases
import chain_scenes as scenes
from conftest import pkg

# ---- the accept / refuse table ------------------------------------------------------------------------------------------
# One row per first stage, one column per (decimation, iqRecord, resampleUp), in the order of chain_cases.matrix():
#   A  accepted: _prepared_settings() returns what chain_cases.prepared_settings() gives
#   R  refused: _prepared_settings() raises ValueError
#   P  passed by: iqRequantize without iqRecord switches nothing on, _prepared_settings() is the settings themselves and the
#      file is read as the int16 / float32 record it is, by the path that prepares nothing
# interferenceMitigation changes no entry: the notch filters whatever int8 record the chain makes, at its rate.
#                      D:   -    -    -    -    D    D    D    D
#                     iq:   -    -    iq   iq   -    -    iq   iq
#                    L/M:   -    r    -    r    -    r    -    r
TABLE = {
    ("none", "int8"):       "A    A    A    A    A    A    A    A",
    ("packed", "int8"):     "A    A    A    A    A    A    A    A",
    ("cond", "int8"):       "A    A    A    A    A    A    A    A",
    ("cond", "uint8"):      "A    A    A    A    A    A    A    A",
    ("cond", "int16"):      "A    A    A    A    A    A    A    A",
    ("requant", "int16"):   "P    R    A    A    R    R    A    A",
    ("requant", "float32"): "P    R    A    A    R    R    A    A",
}
ACCEPTED_CHAINS = 48        # ... of the 56, before the notch doubles them


def verdicts():
    flat = [v for key in cases.FIRST_STAGES for v in TABLE[key].split()]
    chains = cases.matrix()
    assert len(flat) == len(chains) == 56
    return list(zip(chains, flat))


def accepted():
    return [c for c, v in verdicts() if v == "A"]


def test_the_table_counts():
    assert tuple(TABLE) == cases.FIRST_STAGES
    assert len(accepted()) == ACCEPTED_CHAINS
    assert len(set(c.name for c, _ in verdicts())) == 56


@pytest.mark.parametrize("notch", [False, True])
@pytest.mark.parametrize("chain,verdict", verdicts(), ids=[c.name for c, _ in verdicts()])
def test_accept_or_refuse(chain, verdict, notch):
    m = pkg()
    s = chain.settings(m, interferenceMitigation=notch)
    if verdict == "R":
        with pytest.raises(ValueError):
            s._prepared_settings()
        with pytest.raises(ValueError):
            cases.prepared_settings(chain)
        return
    if verdict == "P":
        assert s._prepared_settings() is s and s.dataType == chain.dtype
        with pytest.raises(ValueError):
            cases.prepared_settings(chain)                                     # (the composed contract knows no such chain)
        return
    real = s._prepared_settings()
    want = cases.prepared_settings(chain)
    got = dict((k, getattr(real, k)) for k in want)
    assert got == want, (chain.name, got, want)
    assert not (real.iqRecord or real.decimation or real.resampleUp or real.packedBits or real.frontEndConditioning)
    assert s.samplingFreq == chain.fs and s.IF == chain.f0 and s.dataType == chain.dtype      # the file's settings: left alone


def _variants():
    return list(cases.VARIANTS) + [cases.VARIANT_QI_U8_PLAIN]


@pytest.mark.parametrize("chain", _variants(), ids=[c.name for c in _variants()])
def test_the_variants_are_accepted(chain):
    real = chain.settings(pkg())._prepared_settings()
    want = cases.prepared_settings(chain)
    assert dict((k, getattr(real, k)) for k in want) == want


def test_the_designs_are_the_contracts():
    """The taps the package designs for every accepted chain and variant are the specs' at the rate and carrier the composed
    contract hands each stage - among them the conjugated taps of the Q-first variant and the inverted band of D = 3."""
    m = pkg()
    for chain in accepted() + _variants():
        s = chain.settings(m)
        r = cases.rates(chain)
        if chain.D:
            front = s._walk(upto="decimate")[1] if chain.first == "packed" else s
            taps, shift, info = front._decim_design()
            h, S, fs_out, f_out, inverted = r["decim"]
            assert taps.tobytes() == h.tobytes() and shift == S, chain.name
            assert (info["fs_out"], info["f_out"], info["inverted"]) == (fs_out, f_out, inverted), chain.name
        if chain.resamp:
            taps, shift, info = s._resamp_design()
            h, S, fs_out = r["resamp"]
            assert np.asarray(taps).tobytes() == h.tobytes() and shift == S and info["fs_out"] == fs_out, chain.name
    assert cases.rates(cases.VARIANT_INVERTED)["decim"][4] is True


# ---- the skip mapping ---------------------------------------------------------------------------------------------------

def _splits(chain):
    """{what it splits: skipNumberOfBytes} - each way a skip of this chain can split something."""
    w = 1 if chain.first in ("none", "packed") else np.dtype(chain.dtype).itemsize
    out = {}
    if w > 1:
        out["component"] = w + 1
    if chain.first == "packed":
        if chain.frame * chain.bits > 8:
            out["frame"] = 1
        return out
    if chain.iq:
        out["pair"] = w
    if chain.D:
        out["group of D"] = w * chain.lanes
    if chain.resamp and chain.resamp[1] > 1:
        out["multiple of M"] = w * chain.lanes * (chain.D or 1)
    return out


@pytest.mark.parametrize("chain", accepted() + _variants(), ids=[c.name for c in accepted() + _variants()])
def test_skip_mapping(chain):
    """Every skipNumberOfBytes up to two units and one byte: the legal ones map to the contract's sample, the others are
    refused with the setting's name; the smallest legal one is the contract's unit, and every way the chain's skip can split
    something is among the refused."""
    m = pkg()
    unit = cases.skip_unit(chain)
    legal = []
    tried = list(range(0, 2 * unit + 2)) + [1237 * unit, 1237 * unit + 1]
    for skip in tried:
        s = chain.settings(m, skipNumberOfBytes=skip)
        try:
            want = cases.prepared_skip(chain, skip)
        except ValueError:
            with pytest.raises(ValueError, match="skipNumberOfBytes"):
                s._prepared_settings()
            continue
        legal.append(skip)
        assert s._prepared_settings().skipNumberOfBytes == want, (chain.name, skip)
        assert s.skipNumberOfBytes == skip                                      # left alone
    assert legal == [skip for skip in tried if skip % unit == 0], (chain.name, unit, legal)
    for what, skip in _splits(chain).items():
        assert skip not in legal and 0 < skip < 2 * unit, (chain.name, what, skip)
    # where the unit maps to: the smallest step of the prepared record that is whole at every stage
    step = cases.prepared_skip(chain, unit)
    assert step > 0 and cases.prepared_skip(chain, 2 * unit) == 2 * step


# ---- offsets of the prepared record: refused before anything is uploaded ---------------------------------------------------

@pytest.mark.parametrize("chain", accepted() + _variants(), ids=[c.name for c in accepted() + _variants()])
def test_illegal_offsets_are_refused_before_the_file_is_touched(chain):
    """Every offset below two legal steps that the contract cannot map to the file - off a multiple of L, inside an I/Q
    pair, inside a frame of the packed file - is a ValueError of _prepared_record, with a path that does not exist: nothing
    was opened, nothing uploaded."""
    m = pkg()
    s = chain.settings(m)
    step = cases.prepared_skip(chain, cases.skip_unit(chain))
    refused = 0
    for offset in range(1, 2 * step + 2):
        try:
            cases.file_range(chain, offset, 1000)
        except ValueError:
            refused += 1
            with pytest.raises(ValueError):
                with s._prepared_record("/nonexistent/record.bin", offset, 1000):
                    pass
    if chain.iq or chain.resamp or (chain.first == "packed" and not chain.D and not chain.resamp):
        assert refused > 0, chain.name


@pytest.mark.parametrize("chain", accepted() + _variants(), ids=[c.name for c in accepted() + _variants()])
def test_file_range(chain):
    """The walk back, without a card: Settings._file_range(offset, count) is the contract's file_range() - or both refuse -
    for every offset up to two legal steps and one far beyond, an even, an odd and an off-step count; and it undoes the
    walk forwards: the sample a legal skipNumberOfBytes becomes is made of the file from that byte on."""
    m = pkg()
    s = chain.settings(m)
    unit = cases.skip_unit(chain)
    step = cases.prepared_skip(chain, unit)
    legal = 0
    for offset in list(range(0, 2 * step + 2)) + [1237 * step, 1237 * step + 1]:
        for count in (1000, 1001, step + 1):
            try:
                want = cases.file_range(chain, offset, count)
            except ValueError:
                with pytest.raises(ValueError):
                    s._file_range(offset, count)
                continue
            legal += 1
            assert s._file_range(offset, count) == want, (chain.name, offset, count)
    assert legal >= 9, chain.name                                               # offsets 0, step, 2 step at the least
    for skip in range(0, 2 * unit + 1):
        try:
            want = cases.prepared_skip(chain, skip)
        except ValueError:
            continue
        s.skipNumberOfBytes = skip
        assert s._prepared_settings().skipNumberOfBytes == want
        assert s._file_range(want, 1)[0] == skip, (chain.name, skip)


def test_an_offset_that_splits_a_pair_names_the_pair():
    """The refusal this contract brought: an odd sample of the converter's record - also where decimation by an even D
    would turn it into an even byte of the file - and the sample an offset on a multiple of L maps to."""
    m = pkg()
    for chain, offset in ((cases.matrix_chain("none", "int8", False, True, False), 7),
                          (cases.matrix_chain("none", "int8", True, True, False), 7),
                          (cases.matrix_chain("cond", "int16", False, True, False), 1),
                          (cases.matrix_chain("requant", "float32", True, True, False), 3),
                          (cases.matrix_chain("none", "int8", False, True, True), 5),       # L = 5 -> sample M = 3
                          (cases.matrix_chain("cond", "uint8", True, True, True), 15)):
        with pytest.raises(ValueError, match="splits an I/Q pair"):
            with chain.settings(m)._prepared_record("/nonexistent/record.bin", offset, 1000):
                pass


# ---- the inputs of the notch tests --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chain", accepted(), ids=[c.name for c in accepted()])
def test_the_line_files_are_well_conditioned(chain):
    """The file tests/test_chain_gpu.py gives each chain that ends in the notch, through the composed contract and the
    oracle's spectrum: one line, where the file put it, and no bin within 1 dB of notchThresholdDb."""
    m = pkg()
    s = chain.settings(m)
    b = cases.line_file(chain, np.random.default_rng(cases.LINE_SEED),
                        cases.file_components(chain, cases.prepared_size(chain, m._native)))
    composed = cases.prepare(b, chain, 0, cases.prepared_length(chain, b.size))
    lines, taps = cases.notch_contract(chain, composed, cases.smallest_offset(chain), s.notchThresholdDb, s.notchWidthHz,
                                       s.notchTaps)
    assert len(lines) == 1 and taps.size == s.notchTaps


# ---- the two end-to-end scenes, pinned on the composed contract and the oracle alone -----------------------------------------

@pytest.mark.parametrize("name", sorted(scenes.SCENES))
def test_scenes_are_well_conditioned(name):
    """The composed contract's record of each scene under the oracle's search, in both windows the GPU tests acquire in (at
    the start and behind the skip): exactly the scene's satellites, each at least MARGIN above the threshold, every one of
    the 28 absent PRNs at or below ABSENT_MAX - and the sums of magnitudes that keep tracking on its fastest kernel."""
    scene = scenes.SCENES[name]
    m = pkg()
    o = scene.oracle_settings()
    real = scene.settings(m)._prepared_settings()
    assert (real.samplingFreq, real.IF, real.samplesPerCode) == (o.samplingFreq, o.IF, o.samplesPerCode)
    assert real.samplingFreq > 15.4 * 1023000.0                                # the rate the chain exists for
    y = scenes.prepared(scene, scenes.ACQ_MS)["record"]
    a = np.abs(y.astype(np.int64))
    win = np.concatenate(([0], np.cumsum(a)))
    print("%s: %d samples, rms %.2f, max |y| %d, largest 2048-sample sum of magnitudes %d"
          % (name, y.size, float(np.sqrt(np.mean(y.astype(np.float64) ** 2))), a.max(), (win[2048:] - win[:-2048]).max()))
    assert (win[2048:] - win[:-2048]).max() < 131072
    absent = [p for p in range(1, 33) if p not in scene.prns]
    assert len(absent) == 28
    for skip in (0, scene.skip_bytes):
        assert scene.settings(m, skipNumberOfBytes=skip)._prepared_settings().skipNumberOfBytes == scene.skip_out(skip)
        ref = scenes.contract_acquisition(scene, skip)
        pm = np.asarray(ref["peakMetric"])
        print("%s, skip %d: peak metrics %s, largest among the 28 absent PRNs %.3f"
              % (name, skip, np.round(pm[[p - 1 for p in scene.prns]], 2), float(pm[[p - 1 for p in absent]].max())))
        assert sorted(np.flatnonzero(ref["carrFreq"]) + 1) == sorted(scene.prns)
        assert pm[[p - 1 for p in scene.prns]].min() >= scenes.MARGIN * o.acqThreshold
        assert pm[[p - 1 for p in absent]].max() <= scenes.ABSENT_MAX
