"""The composed contract of the record front end: what Settings._prepared_record(path, offset, count) must yield for a
chain of stages, built only from the numpy contracts of the single stages (tests/unpack_spec.py | cond_spec.py |
requant_spec.py, behind the unpacker or a plain 8-bit file array_spec.py / array_block_spec.py -> decim_spec.py ->
iq_spec.py -> resamp_spec.py), each designed by its own spec at the rate and IF the contract in front of it produced.
The map from (offset, count) to the bytes of the file is written here from what the stages say about themselves - which
sample of an output is which sample of its input - and walks from the prepared record back to the file, stage by stage.
The unit is the slice that is uploaded: a prepared record at an offset is the preparation of that slice (filters start on
zeros, the converter's quarter-rate carrier starts over, the combiner's statistics and blocks are the slice's), not a slice
of the whole file's prepared record.  numpy and the oracle only: no GPU, no package import.  Shared by
tests/test_chain_host.py, tests/test_chain_gpu.py, tests/test_chain_array_host.py and tests/test_chain_array_gpu.py.
Test infrastructure, not product code."""
import numpy as np

import array_block_spec
import array_spec
import cond_spec
import notch_spec
import decim_spec
import iq_spec
import requant_spec
import resamp_spec
import unpack_spec
import waterfall_spec
from oracle import softgnss_oracle as orc

CHIP_RATE = 1023000.0
CODE_LENGTH = 1023
FIRSTS = ("none", "packed", "cond", "requant")


class Chain(object):
    """A plain description of a chain and of the file in front of it.  first: 'none' (an 8-bit file), 'packed' (bits,
    encoding, lsb_first, frame, first_field, peak), 'cond' (dtype int8 / uint8 / int16) or 'requant' (dtype int16 /
    float32); D: the decimation factor or 0; iq, q_first; resamp: (L, M) or None; fs, f0: Settings.samplingFreq and IF of
    the FILE (for I/Q the complex rate and the offset of the carrier from the centre); then the *Taps settings and the
    other knobs of the stages at the package's defaults.  dtype 'uint8' is offset binary, consumed by the first stage
    that sees it.  antennas: the file interleaves that many streams frame by frame (0: one stream) and the combiner stands
    behind the first stage ('none' or 'packed' only), with array_taps (0: 1 for I/Q, else 5), array_reference, array_loading,
    array_target_rms, and with array_block_ms the weights per block of that many ms, from array_window blocks."""

    def __init__(self, first="none", dtype="int8", D=0, iq=False, q_first=False, resamp=None, fs=16368000.0, f0=2000000.0,
                 bits=2, encoding="sign-magnitude", lsb_first=False, frame=1, first_field=0, peak=unpack_spec.DEFAULT_PEAK,
                 iq_taps=iq_spec.DEFAULT_TAPS, decim_taps=decim_spec.DEFAULT_TAPS, decim_bandwidth=decim_spec.DEFAULT_BANDWIDTH,
                 decim_gain=0.0, resamp_taps=0, resamp_cutoff=0.0, resamp_gain=1.0, cond_block_us=100.0, cond_agc_blocks=32.0,
                 cond_blank_factor=4.0, cond_guard=8, cond_target_rms=12.0, requant_target_rms=requant_spec.DEFAULT_TARGET_RMS,
                 notch=False, antennas=0, array_taps=0, array_reference=0, array_loading=array_spec.DEFAULT_LOADING,
                 array_target_rms=array_spec.DEFAULT_TARGET_RMS, array_block_ms=0.0, array_window=3):
        assert first in FIRSTS
        self.first, self.dtype, self.D, self.iq, self.q_first = first, np.dtype(dtype).name, int(D), bool(iq), bool(q_first)
        self.resamp = None if not resamp else (int(resamp[0]), int(resamp[1]))
        self.fs, self.f0 = float(fs), float(f0)
        self.bits, self.encoding, self.lsb_first, self.frame, self.first_field, self.peak = \
            int(bits), encoding, bool(lsb_first), int(frame), int(first_field), int(peak)
        self.iq_taps, self.decim_taps, self.decim_bandwidth, self.decim_gain = int(iq_taps), int(decim_taps), \
            float(decim_bandwidth), float(decim_gain)
        self.resamp_taps, self.resamp_cutoff, self.resamp_gain = int(resamp_taps), float(resamp_cutoff), float(resamp_gain)
        self.cond_block_us, self.cond_agc_blocks, self.cond_blank_factor, self.cond_guard, self.cond_target_rms = \
            float(cond_block_us), float(cond_agc_blocks), float(cond_blank_factor), int(cond_guard), float(cond_target_rms)
        self.requant_target_rms = float(requant_target_rms)
        self.notch = bool(notch)
        self.antennas, self.array_taps, self.array_reference = int(antennas), int(array_taps), int(array_reference)
        self.array_loading, self.array_target_rms = float(array_loading), float(array_target_rms)
        self.array_block_ms, self.array_window = float(array_block_ms), int(array_window)

    @property
    def name(self):
        first = {"none": self.dtype if (self.dtype != "int8" or self.antennas) else "none", "packed": "packed%d" % self.bits,
                 "cond": "cond_" + self.dtype, "requant": "requant_" + self.dtype}[self.first]
        if self.first == "packed" and self.frame > 1:
            first += "_f%d_%d" % (self.frame, self.first_field)
        array = None
        if self.antennas:                                # a3, a3b (per block), a8k1, a2k15ref1
            array = "a%d%s%s%s" % (self.antennas, "b" if self.array_block_ms else "",
                                   "k%d" % self.array_taps if self.array_taps else "",
                                   "ref%d" % self.array_reference if self.array_reference else "")
        parts = [first, array, "d%d" % self.D if self.D else None, ("qi" if self.q_first else "iq") if self.iq else None,
                 "r%d_%d" % self.resamp if self.resamp else None, "notch" if self.notch else None]
        return "-".join(p for p in parts if p)

    @property
    def lanes(self):
        return 2 if self.iq else 1

    def settings(self, m, **kw):
        """The package's settings of the FILE (m: the package)."""
        s = m.Settings()
        s.samplingFreq, s.IF, s.dataType = self.fs, self.f0, self.dtype
        s.iqRecord, s.iqQFirst, s.iqTaps = self.iq, self.q_first, self.iq_taps
        if self.first == "packed":
            s.packedBits, s.packedEncoding, s.packedLsbFirst = self.bits, self.encoding, self.lsb_first
            s.packedFrame, s.packedFirst, s.packedPeak = self.frame, self.first_field, self.peak
        elif self.first == "cond":
            s.frontEndConditioning = True
            s.condBlockUs, s.condAgcBlocks, s.condBlankFactor = self.cond_block_us, self.cond_agc_blocks, self.cond_blank_factor
            s.condGuardFrames, s.condTargetRms = self.cond_guard, self.cond_target_rms
        elif self.first == "requant":
            s.iqRequantize, s.iqTargetRms = True, self.requant_target_rms
        s.decimation, s.decimTaps, s.decimBandwidth, s.decimGain = self.D, self.decim_taps, self.decim_bandwidth, self.decim_gain
        if self.resamp:
            s.resampleUp, s.resampleDown = self.resamp
        s.resampTaps, s.resampCutoff, s.resampGain = self.resamp_taps, self.resamp_cutoff, self.resamp_gain
        s.interferenceMitigation = self.notch
        if self.antennas:
            s.antennas, s.arrayTaps, s.arrayReference = self.antennas, self.array_taps, self.array_reference
            s.arrayLoading, s.arrayTargetRms = self.array_loading, self.array_target_rms
            s.arrayBlockMs, s.arrayWindowBlocks = self.array_block_ms, self.array_window
        for k, v in kw.items():
            setattr(s, k, v)
        return s


# ---- what each stage makes of the format: refusals as ValueError ----------------------------------------------------------

def _first_stage(chain):
    """(w, per_unit, unit): the first stage reads the file in units of `unit` bytes - the smallest run of whole bytes that
    holds whole elements (packed: whole frames) - and makes `per_unit` int8 components of each; w: bytes per component of an
    unpacked file.  Raises ValueError for a first stage that does not read this file."""
    dt = np.dtype(chain.dtype)
    if chain.antennas:
        array_of(chain)
    if chain.first == "packed":
        if dt != np.dtype(np.int8):
            raise ValueError("a packed file is described as int8")
        take = _take(chain)
        unpack_spec.check(chain.bits, int(chain.lsb_first), chain.frame, chain.first_field, take)
        frame_bits = chain.frame * chain.bits
        unit = max(1, frame_bits // 8)
        return 1, (8 * unit // frame_bits) * take, unit
    if chain.first == "cond":
        w, _ = cond_spec.width(dt)                       # (refuses float32)
        return w, 1, w
    if chain.first == "requant":
        if not chain.iq:
            raise ValueError("the requantiser stands in front of the I/Q converter: it reads I/Q files only")
        w = requant_spec.width(dt)                       # (refuses 8-bit types)
        return w, 1, w
    if dt == np.dtype(np.uint8) and (chain.iq or chain.antennas):
        return 1, 1, 1                                   # offset binary: the combiner, the decimator or the converter takes it
    if dt != np.dtype(np.int8):
        raise ValueError("no stage of this chain reads %s" % dt.name)
    return 1, 1, 1


def _take(chain):
    """Fields the unpacker takes of a frame of several: one, with iq the pair, with antennas those of every antenna."""
    take = 2 if (chain.iq and chain.frame > 1) else 1
    return take * chain.antennas if (chain.antennas and chain.frame > 1) else take


def array_of(chain):
    """(A, K, reference, block length in frames or 0, window in blocks) of the combiner, which reads A x lanes components a
    frame and makes lanes of them: output frame f is the instant of input frame f.  ValueError for what it refuses."""
    if chain.first not in ("none", "packed"):
        raise ValueError("a gain per stream would destroy the coherence of the streams: no antennas behind %s" % chain.first)
    if np.dtype(chain.dtype) not in (np.dtype(np.int8), np.dtype(np.uint8)):
        raise ValueError("a multi-antenna record holds int8 or uint8 samples")
    A, K, ref = chain.antennas, chain.array_taps or (1 if chain.iq else 5), chain.array_reference
    array_spec.check_shape(chain.lanes, A, K)
    if not (0 <= ref < A):
        raise ValueError("the reference is one of the antennas")
    if not (np.isfinite(chain.array_loading) and chain.array_loading >= 0 and 0 < chain.array_target_rms <= 127.0):
        raise ValueError("loading and target rms")
    W = chain.array_window
    if not (1 <= W <= array_block_spec.MAX_WINDOW and W % 2 == 1):
        raise ValueError("the window is an odd number of blocks")
    if not (np.isfinite(chain.array_block_ms) and chain.array_block_ms >= 0):
        raise ValueError("the block length")
    B = 0
    if chain.array_block_ms:                             # to a whole multiple of the unit, at the rate of frames
        unit = array_block_spec.BLOCK_UNIT
        B = max(1, int(round(chain.array_block_ms * chain.fs / 1000.0 / unit))) * unit
    return A, K, ref, B, W


def _frame(chain):
    """Components of a frame in front of the decimator's input: of all antennas where there are several."""
    return chain.lanes * (chain.antennas or 1)


def _whole(chain):
    """(per_unit, unit) of the least run of file bytes that holds whole units of the first stage and, with antennas, whole
    frames of all antennas: the upload is rounded up to it, and of a packed file that ends early it is what is kept."""
    w, per_unit, unit = _first_stage(chain)
    k = int(np.lcm(per_unit, _frame(chain))) // per_unit if chain.antennas else 1
    return k * per_unit, k * unit


def _offset_binary_behind_first(chain):
    """Whether the int8 record behind the first stage and the combiner still is offset binary: only where no stage has
    touched the file - the combiner takes it."""
    return chain.first == "none" and chain.dtype == "uint8" and not chain.antennas


def rates(chain):
    """The rates along the chain: dict with decim (taps, shift, fs_out, f_out, inverted) or None, the rate and carrier in
    front of the converter (fs_front, f_front), resamp (taps, shift, fs_out) or None, and the prepared record's fs, IF.
    ValueError where a stage's design refuses."""
    _first_stage(chain)
    out = dict(decim=None, resamp=None)
    fs, f0 = chain.fs, chain.f0
    if chain.D:
        h, S, fs, f0, inverted = decim_spec.design(fs, f0, chain.decim_bandwidth, chain.lanes, chain.D, chain.decim_taps,
                                                   chain.decim_gain)
        if chain.iq and chain.q_first:
            h = h.copy()
            h[1::2] = -h[1::2]           # a Q-first file is Q + jI: conj(h) makes Im w + j Re w of it, Q first again
        out["decim"] = (h, S, fs, f0, inverted)
    out["fs_front"], out["f_front"] = fs, f0
    if chain.iq:
        fs, f0 = iq_spec.real_equivalent(fs, f0)
    if chain.resamp:
        L, M = chain.resamp
        h, S, fs_out = resamp_spec.design(fs, L, M, chain.resamp_taps, chain.resamp_cutoff, chain.resamp_gain)
        cutoff = chain.resamp_cutoff if chain.resamp_cutoff else resamp_spec.default_cutoff(fs, L, M)
        if not f0 + CHIP_RATE < cutoff:
            raise ValueError("the resampler's low-pass cuts into the C/A band")
        out["resamp"] = (h, S, fs_out)
        fs = fs_out
    out["fs"], out["IF"] = fs, f0
    return out


def samples_per_code(fs):
    """The reference's samplesPerCode: round(fs / (codeFreqBasis / codeLength)), half to even."""
    return int(round(fs / (CHIP_RATE / CODE_LENGTH)))


# ---- positions: which sample of the prepared record is which byte of the file ---------------------------------------------

def skip_unit(chain):
    """The smallest legal non-zero skipNumberOfBytes of the chain: the least run of file bytes that is whole units of the
    first stage, whole frames of all antennas, whole pairs, whole groups of D frames and whole groups of M samples in
    front of the resampler at once."""
    w, per_unit, unit = _first_stage(chain)
    need = chain.lanes * (chain.D or 1)                  # components: a group of D frames
    if chain.resamp:
        need = np.lcm(need, chain.resamp[1] * (chain.D or 1))   # ... M samples behind the decimator are M D in front of it
    need = int(need) // chain.lanes * _frame(chain)      # ... of the combiner's output are frames of all antennas in front of it
    units = int(np.lcm(int(need), per_unit)) // per_unit
    return units * unit


def walk(chain):
    """[(stage, n_in, n_out)] in the chain's order, as Settings._walk() names them: n_in positions of what the stage reads
    become n_out of what it writes."""
    w, per_unit, unit = _first_stage(chain)
    steps = [({"packed": "unpack", "cond": "condition", "requant": "requantise"}[chain.first], unit, per_unit)] \
        if chain.first != "none" else []
    if chain.antennas:
        steps.append(("combine", _frame(chain), chain.lanes))
    if chain.D:
        steps.append(("decimate", chain.lanes * chain.D, chain.lanes))
    if chain.iq:
        steps.append(("convert", 2, 2))
    if chain.resamp:
        steps.append(("resample", chain.resamp[1], chain.resamp[0]))
    return steps


def prepared_skip(chain, skip_bytes):
    """The sample of the prepared record that byte skip_bytes of the file becomes, walking forwards; ValueError where the
    byte does not begin a sample of every record along the chain."""
    w, per_unit, unit = _first_stage(chain)
    skip_bytes = int(skip_bytes)
    if skip_bytes % unit:
        raise ValueError("the byte splits %s" % ("a frame" if chain.first == "packed" else "a component"))
    pos = skip_bytes // unit * per_unit                  # component of the int8 record behind the first stage
    if chain.antennas:
        if pos % _frame(chain):
            raise ValueError("the byte splits a frame of all antennas")
        pos = pos // _frame(chain) * chain.lanes         # output frame f is input frame f
    if pos % chain.lanes:
        raise ValueError("the byte splits an I/Q pair")
    if chain.D:
        frame = pos // chain.lanes
        if frame % chain.D:
            raise ValueError("the byte splits a group of D frames")
        pos = frame // chain.D * chain.lanes             # output frame m is input frame m D
    if chain.resamp:                                     # (the converter keeps positions: byte n is the instant of byte n's pair)
        L, M = chain.resamp
        if pos % M:
            raise ValueError("the sample is not one of the resampled record")
        pos = pos // M * L                               # output n L is input n M
    return pos


def prepared_settings(chain, skip_bytes=0):
    """What _prepared_settings() must return: dict(samplingFreq, IF, dataType, skipNumberOfBytes, samplesPerCode)."""
    r = rates(chain)
    return dict(samplingFreq=r["fs"], IF=r["IF"], dataType="int8", skipNumberOfBytes=prepared_skip(chain, skip_bytes),
                samplesPerCode=samples_per_code(r["fs"]))


def file_range(chain, offset, count):
    """(first byte, bytes) of the file that samples [offset, offset + count) of the prepared record are made of, walking
    backwards from the prepared record to the file.  ValueError where `offset` is not a sample of every record on the way."""
    w, per_unit, unit = _first_stage(chain)
    start, n = int(offset), int(count)
    if chain.resamp:
        L, M = chain.resamp
        # output m is the instant m M / L of the input: output k L is input k M, and `n` outputs from there span n M / L
        # input samples - every input sample that starts inside that span is read
        if start % L:
            raise ValueError("sample %d of the resampled record is no sample of the record in front of the resampler" % start)
        start = start // L * M
        n = len(range(0, n * M, L))
        if chain.iq:
            n += n & 1                                   # the converter makes whole pairs
    if chain.iq and (start % 2):
        raise ValueError("sample %d starts inside an I/Q pair" % start)
    if chain.D:                                          # frame m of the decimated record is frame m D of its input
        start = (start // chain.lanes) * chain.D * chain.lanes
        n = n * chain.D
    if chain.antennas:                                   # frame f of the combined record is frame f of all antennas
        if start % chain.lanes:
            raise ValueError("sample %d starts inside a frame" % start)
        start = start // chain.lanes * _frame(chain)
        n = -(-n * _frame(chain) // chain.lanes)
    if start % per_unit:
        raise ValueError("sample %d does not start a frame of the packed file" % start)
    first = start // per_unit * unit
    if chain.first == "packed":
        per_unit, unit = _whole(chain)                   # (with antennas: whole frames of all of them too)
    units = (n + per_unit - 1) // per_unit               # whole units: a packed file is read frame by frame
    return first, units * unit


def components_per_unit(chain):
    """(components the first stage makes of one unit of the file, bytes of that unit); with antennas the components of the
    combined record that the least run of whole units and whole frames of all antennas becomes (an unpacked file: a
    component of the combined record is `antennas` bytes)."""
    _, per_unit, unit = _first_stage(chain)
    if chain.antennas:
        if chain.first != "packed":
            return 1, chain.antennas
        per_unit, unit = _whole(chain)
        return per_unit // chain.antennas, unit
    return per_unit, unit


def prepared_length(chain, n_bytes):
    """Samples of the prepared record of a file of n_bytes bytes (whole units), walking forwards."""
    per_unit, unit = _whole(chain)
    n = int(n_bytes) // unit * per_unit
    if chain.antennas:
        n = n // _frame(chain) * chain.lanes
    if chain.D:
        n = -(-(n // chain.lanes) // chain.D) * chain.lanes
    if chain.resamp:
        n = resamp_spec.out_length(n, chain.resamp[0], chain.resamp[1])
    return n


def rounding_unit(chain):
    """The most by which len(prepared record) may exceed `count`, in samples of the prepared record: the upload is rounded
    up to whole frames of a packed file (at most per_unit - 1 components more; behind the decimator a part of a group of D
    frames still gives a frame), to whole pairs in front of the resampler (1 more), and to whole input samples of the
    resampler: with n_in < count M / L + 1 + e input samples it makes fewer than count + (1 + e) L / M."""
    w, per_unit, unit = _first_stage(chain)
    extra = per_unit - 1                                 # components behind the first stage
    if chain.antennas:                                   # whole frames of all antennas too: at most one such run less a
        extra = _whole(chain)[0] // chain.antennas - 1   # component, `antennas` of them to one of the combined record
    if chain.D:
        extra = chain.lanes * -(-(-(-extra // chain.lanes)) // chain.D)
    if chain.resamp:
        L, M = chain.resamp
        extra = -(-(extra + 1 + (1 if chain.iq else 0)) * L // M)
    return max(extra, chain.lanes - 1)                   # (an odd count in front of the converter: a whole pair)


# ---- the composition --------------------------------------------------------------------------------------------------

FLAWS = ("swap", "grid", "offset_binary", "file_stats", "first_field")


def _combine(chain, x, flags, flaw=None, x_file=None, at=0):
    """The combiner's contract on the int8 record x that interleaves the antennas: (record, out["combine"]).  The statistics
    and, per block, the blocks are those of x itself: blocks count from its first frame.  flaw, for tests/test_chain_array_host.py
    only: 'swap' runs two antennas that are not the reference through each other's taps, 'grid' counts the blocks from one
    frame early, 'file_stats' takes the statistics (per block: the grid) of x_file, the whole file's record, of which x is
    the frames from `at` on."""
    A, K, ref, B, W = array_of(chain)
    lanes, w = chain.lanes, _frame(chain)
    frames = x.size // w
    if not B:
        src, n = (x_file, x_file.size // w) if flaw == "file_stats" else (x, frames)
        rho = array_spec.stats(src, lanes, A, K, flags)
        taps, shift, gain, supp, weights = array_spec.design(rho, n, lanes, ref, chain.array_loading, chain.array_target_rms)
        if flaw == "swap":
            i, j = [a for a in range(A) if a != ref][:2]
            taps = taps.copy()
            taps[[i, j]] = taps[[j, i]]
        y, clipped = array_spec.combine(x, taps, shift, lanes, A, flags)
        return y, dict(samples=y.size, clipped=clipped, weights=weights, suppression_db=supp, gain=gain, taps=taps)
    lead = 0
    if flaw == "grid":                                   # a frame of zeros in front: every block begins a frame early
        zero = np.full(w, -128 if flags else 0, dtype=np.int8)
        x, lead = np.concatenate([zero, x]), 1
    elif flaw == "file_stats":
        x, lead = x_file, at
    n = x.size // w
    rho = array_block_spec.block_stats(x, lanes, A, K, B, flags)
    taps, shift, gain, supp, weights, status = array_block_spec.design_blocks(rho, n, B, W, lanes, ref, chain.array_loading,
                                                                              chain.array_target_rms)
    if flaw == "swap":
        i, j = [a for a in range(A) if a != ref][:2]
        taps = taps.copy()
        taps[:, [i, j]] = taps[:, [j, i]]
    y, clipped = array_block_spec.combine_blocks(x, taps, B, shift, lanes, A, flags)
    y = y[lead * lanes:(lead + frames) * lanes]
    return y, dict(samples=y.size, clipped=clipped, weights=weights, suppression_db=supp, gain=gain, taps=taps,
                   blocks=int(rho.shape[0]), block_frames=B, held=int(np.count_nonzero(status)), status=status)


def prepare(file_bytes, chain, offset, count, requant_sums=None, flaw=None):
    """What _prepared_record(path, offset, count) must yield for a file holding file_bytes: dict with `record` (int8), per
    stage that ran a dict of the contract's counts - unpack (samples, code_counts), cond (samples, block, blocks, blanked
    frames, clipped), requant (samples, clipped, mult, shift, scale), decim (samples, clipped, fs_out, f_out, inverted),
    resamp (samples, clipped, fs_out) - and the prepared (fs, IF).  A file that ends inside the range is read as far as it
    goes; of a packed file whole frames are kept; any other file must then end on whole elements and pairs (ValueError from
    the stage's contract otherwise).  requant_sums: (n_finite, sum_sq) as the library summed a float32 file, which its
    contract lets differ from the correctly rounded sums by requant_spec.bounds(); None: the contract's own.  With antennas
    combine: samples, clipped, weights, suppression_db, gain (per block arrays, the blocks counted from the slice's first
    frame) and per block blocks, block_frames, held, status; a packed file then keeps whole frames of all antennas.  flaw: one
    of FLAWS, a deliberate mistake of the composition, for the tests that show the inputs would expose it."""
    assert flaw is None or (flaw in FLAWS and chain.antennas)
    raw = np.ascontiguousarray(file_bytes).view(np.uint8).ravel()
    w, per_unit, unit = _first_stage(chain)
    r = rates(chain)
    first, n_bytes = file_range(chain, offset, count)
    b = raw[first:first + n_bytes]
    out = dict(fs=r["fs"], IF=r["IF"], file_range=(first, b.size))
    x_file = None
    if chain.first == "packed":
        whole = _whole(chain)[1]
        b = b[:b.size // whole * whole]                  # a frame the file ends in is left
        out["file_range"] = (first, b.size)
        take = _take(chain)
        table = unpack_spec.table(chain.bits, unpack_spec.ENCODINGS[chain.encoding], chain.peak)
        flags = unpack_spec.LSB_FIRST if chain.lsb_first else 0
        field = chain.first_field
        if flaw == "first_field":
            field = field + 1 if field + 1 + take <= chain.frame else field - 1
            assert chain.frame > 1 and field >= 0
        x = unpack_spec.unpack(b, chain.bits, table, flags, chain.frame, field, take)
        if flaw == "file_stats":
            x_file = unpack_spec.unpack(raw[:raw.size // whole * whole], chain.bits, table, flags, chain.frame, field, take)
        out["unpack"] = dict(samples=x.size, table=table,
                             code_counts=unpack_spec.code_counts(b, chain.bits, flags, chain.frame, chain.first_field, take))
    elif chain.first == "cond":
        block = cond_spec.block_frames(chain.fs, chain.cond_block_us)
        q4 = cond_spec.blank_q4_of(chain.cond_blank_factor)
        stats = cond_spec.block_stats(b, chain.dtype, chain.lanes, block, q4)
        plan = cond_spec.plan(stats, chain.lanes, q4, chain.cond_target_rms, chain.cond_agc_blocks)
        x, blanked, clipped = cond_spec.condition(b, chain.dtype, chain.lanes, block, plan, chain.cond_guard)
        out["cond"] = dict(samples=x.size, block=block, blocks=int(plan.size), blanked=blanked, clipped=clipped)
    elif chain.first == "requant":
        st = requant_spec.stats(b, chain.dtype)
        n_finite, sum_sq = (st["n_finite"], st["sum_sq"]) if requant_sums is None else requant_sums
        mult, shift, scale = requant_spec.gain(n_finite, sum_sq, chain.requant_target_rms)
        x = requant_spec.quantise(b, chain.dtype, mult, shift, scale)
        out["requant"] = dict(samples=x.size, clipped=int(np.count_nonzero(np.abs(x.astype(np.int16)) == 127)), mult=mult,
                              shift=shift, scale=scale, stats=st)
    else:
        x = b.view(np.int8)
        x_file = raw.view(np.int8)
    ob = _offset_binary_behind_first(chain)
    if chain.antennas:
        taken = chain.first == "none" and chain.dtype == "uint8"           # the combiner takes the offset binary
        x, out["combine"] = _combine(chain, x, array_spec.OFFSET_BINARY if taken else 0, flaw, x_file,
                                     first // unit * per_unit // _frame(chain))
        ob = taken and flaw == "offset_binary"
    if chain.D:
        h, S, fs_out, f_out, inverted = r["decim"]
        x, clipped = decim_spec.decimate(x, h, S, chain.lanes, chain.D, decim_spec.OFFSET_BINARY if ob else 0)
        ob = False
        out["decim"] = dict(samples=x.size, clipped=clipped, fs_out=fs_out, f_out=f_out, inverted=inverted)
    if chain.iq:
        h, S = iq_spec.design(chain.iq_taps)
        x = iq_spec.convert(x, h, S, (iq_spec.Q_FIRST if chain.q_first else 0) | (iq_spec.OFFSET_BINARY if ob else 0))
    if chain.resamp:
        h, S, fs_out = r["resamp"]
        x, clipped = resamp_spec.resample(x, h, S, chain.resamp[0], chain.resamp[1])
        out["resamp"] = dict(samples=x.size, clipped=clipped, fs_out=fs_out)
    out["record"] = np.ascontiguousarray(x).view(np.int8)
    return out


# ---- the matrix of tests/test_chain_host.py and tests/test_chain_gpu.py ----------------------------------------------------
# Files at 4 to 16 Msps, so that ten code periods of every prepared record stay in the hundreds of kilobytes: a real file at
# 16.368 Msps with the carrier at 2 MHz (decimated by 2: 8.184 Msps, the band upright in the first Nyquist zone); an I/Q file
# at 4.092 Msps, the carrier 0.2 MHz off centre (converted: 8.184 Msps, IF 2.246 MHz), or where it is decimated by 2 at
# 8.184 Msps, the carrier 1 MHz below centre (decimated and converted: 8.184 Msps, IF 1.046 MHz).  Every one of these leaves
# the C/A band below the cutoff of a 5/3 resampler.
REAL_FILE = (16368000.0, 2000000.0)
IQ_FILE = (4092000.0, 200000.0)
IQ_FILE_DECIMATED = (8184000.0, -1000000.0)
MATRIX_D = 2
MATRIX_RESAMP = (5, 3)      # M = 3: a pair, a group of D and a multiple of M are three different things
FIRST_STAGES = (("none", "int8"), ("packed", "int8"), ("cond", "int8"), ("cond", "uint8"), ("cond", "int16"),
                ("requant", "int16"), ("requant", "float32"))


def matrix_chain(first, dtype, D, iq, resamp, notch=False, **kw):
    fs, f0 = (IQ_FILE_DECIMATED if D else IQ_FILE) if iq else REAL_FILE
    return Chain(first=first, dtype=dtype, D=MATRIX_D if D else 0, iq=iq, resamp=MATRIX_RESAMP if resamp else None, fs=fs,
                 f0=f0, notch=notch, **kw)


def matrix():
    """Every combination of first stage x decimation x iqRecord x resampleUp, in a fixed order: 56 chains."""
    return [matrix_chain(first, dtype, D, iq, res) for first, dtype in FIRST_STAGES for D in (False, True)
            for iq in (False, True) for res in (False, True)]


# the variants: one chain each, not multiplied across the matrix
VARIANT_QI_U8 = Chain(dtype="uint8", D=4, iq=True, q_first=True, resamp=(3, 1), fs=16368000.0, f0=3200000.0)
VARIANT_QI_U8_PLAIN = Chain(dtype="int8", D=4, iq=True, q_first=False, resamp=(3, 1), fs=16368000.0, f0=3200000.0)
VARIANT_FRAME = Chain(first="packed", bits=2, frame=4, first_field=1, D=2, fs=REAL_FILE[0], f0=REAL_FILE[1])
VARIANT_FRAME_IQ = Chain(first="packed", bits=4, frame=8, first_field=2, lsb_first=True, encoding="offset-binary", D=2,
                         iq=True, fs=IQ_FILE_DECIMATED[0], f0=IQ_FILE_DECIMATED[1])
VARIANT_INVERTED = Chain(D=3, resamp=(7, 3), fs=38192000.0, f0=9548000.0)
VARIANTS = (VARIANT_QI_U8, VARIANT_FRAME, VARIANT_FRAME_IQ, VARIANT_INVERTED)


def full_scale_file(chain, rng, components):
    """The bytes of a file of `components` components (packed: fields) that drives the chain's first stage over its whole
    range: every byte value for 8-bit and packed files (all codes, both rails), both int16 rails, and for float32 the int8
    full-scale values at 3.4e-5 of their size.  A multi-antenna chain's file is array_file()'s: random bytes would let any
    combiner pass."""
    n = int(components)
    if chain.antennas:
        return array_file(chain, rng, n, zero_blocks=ARRAY_ZERO_BLOCKS.get(chain.name), line=chain.notch)
    if chain.first == "packed":
        assert (n * chain.bits) % 8 == 0
        b = rng.integers(0, 256, n * chain.bits // 8).astype(np.uint8)
        b[:256] = rng.permutation(256)
        return b
    dt = np.dtype(chain.dtype)
    if dt.itemsize == 1:
        x = rng.integers(-128, 128, n).astype(np.int8)
        x[::97], x[5::101] = -128, 127
        return x.view(np.uint8)
    if dt == np.dtype(np.int16):
        x = rng.integers(-32768, 32768, n).astype("<i2")
        x[::97], x[5::101] = -32768, 32767
        return x.view(np.uint8)
    x = rng.integers(-128, 128, n).astype(np.int8)
    x[::97], x[5::101] = -128, 127
    return (x.astype(np.float32) * np.float32(3.4e-5)).astype("<f4").view(np.uint8)


def file_components(chain, prepared_samples):
    """Components (packed: fields) of a file whose prepared record holds at least prepared_samples samples, to whole
    skip units."""
    first, n_bytes = file_range(chain, 0, prepared_samples)
    u = skip_unit(chain)
    n_bytes = -(-n_bytes // u) * u
    if chain.first == "packed":
        return n_bytes * 8 // chain.bits
    return n_bytes // np.dtype(chain.dtype).itemsize


# ---- multi-antenna chains: the files, the matrix, the variants ------------------------------------------------------------
# Random bytes give every antenna but the reference taps that round to nothing, and any combiner passes.  These files hold a
# strong component common to all streams - a gain, a sign (I/Q: a phase) and a delay of its own per stream, the gain drifting
# along the file so that the weights of a slice are not the file's and those of a block not its neighbour's -, a weaker
# second one with other gains, so that no stream is a multiple of another, and independent noise.
ARRAY_STRONG, ARRAY_WEAK, ARRAY_NOISE = 24.0, 8.0, 5.0          # LSB per component
ARRAY_DRIFT = 0.4                                               # the strong component's gain swings by that share
ARRAY_GAINS = (1.0, -0.8, 0.6, 0.9, -0.7, 0.5, 0.85, -0.95)     # of the strong component, per stream, ...
ARRAY_GAINS_WEAK = (0.7, 1.0, -0.9, -0.5, 0.8, -1.0, 0.6, 0.9)  # ... and of the weak one
ARRAY_STEP = {1: 1.0, 2: 1.0, 4: 0.34}                          # a packed file's quantiser step, in units of the rms
ARRAY_LINE_AMPLITUDE = 1.5      # the line of a chain that ends in the notch: under the noise of every antenna, and with a
                                # phase of its own per antenna - a line in phase on all of them is one more common
                                # component, which the power inversion takes out with the others
ARRAY_SEED = 0xC4A1             # (the seed tests/test_chain_gpu.py's run_chain writes its files with)


def array_file(chain, rng, components, zero_blocks=None, line=False):
    """The bytes of a multi-antenna file of `components` components (packed: fields) as described above, with runs of both
    rails on all streams and on single ones and every byte value in the first 256 bytes; uint8: the same samples in offset
    binary; packed: quantised with ARRAY_STEP and packed through unpack_spec.  A packed frame of more fields than the
    antennas take holds further streams of the same kind.  zero_blocks (j0, j1): the frames of blocks j0 .. j1 - 1 are all
    zero.  line: with the line of line_frequency(), ARRAY_LINE_AMPLITUDE high."""
    A, K, ref, B, W = array_of(chain)
    lanes = chain.lanes
    per_frame = chain.frame if (chain.first == "packed" and chain.frame > 1) else A * lanes
    n = int(components)
    assert n % per_frame == 0 and per_frame % lanes == 0
    F, streams = n // per_frame, per_frame // lanes
    assert streams <= len(ARRAY_GAINS)
    t = np.arange(F, dtype=np.float64)

    def common():                                        # a complex envelope, smoothed over three frames
        z = rng.standard_normal(F + 4) + 1j * rng.standard_normal(F + 4)
        return (z[:-2] + 2.0 * z[1:-1] + z[2:]) / np.sqrt(6.0)
    strong, weak = common(), common()
    v = np.empty((F, streams, lanes))
    for a in range(streams):
        drift = 1.0 + ARRAY_DRIFT * np.sin(2.0 * np.pi * 1.5 * t / F + a)
        d = a % 3 if lanes == 1 else 0                   # the delay, frames (one tap per antenna takes none out)
        z = ARRAY_STRONG * ARRAY_GAINS[a] * drift * np.exp(0.7j * a * a * (lanes - 1)) * strong[d:d + F]
        z = z + ARRAY_WEAK * ARRAY_GAINS_WEAK[a] * np.exp(-1.3j * a * (lanes - 1)) * weak[2 - d:2 - d + F]
        z = z + ARRAY_NOISE * (rng.standard_normal(F) + 1j * rng.standard_normal(F))
        if line:
            z = z + ARRAY_LINE_AMPLITUDE * np.exp(1j * (2.0 * np.pi * line_frequency(chain)[1] * t / chain.fs + 2.4 * a))
        v[:, a, 0] = z.real
        if lanes == 2:
            v[:, a, 1] = z.imag
    v = v.reshape(F, per_frame)
    if chain.first == "packed":
        half = 1 << (chain.bits - 1)
        step = ARRAY_STEP[chain.bits] * float(np.sqrt(np.mean(v * v)))
        idx = np.clip(np.floor(v / step) + half, 0, 2 * half - 1).astype(np.int64)
        for k, p in enumerate(range(1000, F - 8, max(1, F // 7))):             # runs of both rails
            idx[p:p + 5] = 0 if k % 2 else 2 * half - 1
            idx[p + 40:p + 47, k % per_frame] = 2 * half - 1 if k % 2 else 0
        code = unpack_spec.code_of_level(chain.bits, unpack_spec.ENCODINGS[chain.encoding])[idx.reshape(-1)]
        b = unpack_spec.pack(code, chain.bits, unpack_spec.LSB_FIRST if chain.lsb_first else 0)
        b[:256] = rng.permutation(256)
        return b
    x = np.clip(np.rint(v), -128, 127).astype(np.int8)
    for k, p in enumerate(range(1000, F - 8, max(1, F // 7))):
        x[p:p + 5] = 127 if k % 2 else -128
        x[p + 40:p + 47, k % per_frame] = -128 if k % 2 else 127
    if zero_blocks:
        x[zero_blocks[0] * B:zero_blocks[1] * B] = 0
    x = x.reshape(-1)
    x[:256] = (rng.permutation(256) - 128).astype(np.int8)
    return x.view(np.uint8) ^ np.uint8(0x80 if chain.dtype == "uint8" else 0)


ARRAY_FIRST_STAGES = (("none", "int8"), ("none", "uint8"), ("packed", "int8"))
ARRAY_BLOCK_FRAMES = 4096
# arrayTargetRms per family, so that the contract's combined record clips more than none and fewer than 1 % of its samples
# (tests/test_chain_array_host.py asserts it): what is left behind the null is close to Gaussian, which leaves +-127 with
# 0.15 % of its samples at an rms of 40 LSB, and the rails of the files add to that.  The chain with the stretch of zeros
# takes 22: a window of which two blocks in three are zero designs 1.7 times the gain, and its taps must stay taps
ARRAY_TARGET_RMS = {"none": 40.0, "packed": 40.0, "hold": 22.0}


def array_chain(first, dtype, D, iq, resamp, antennas=3, block=False, **kw):
    """A multi-antenna chain at the matrix's rates; a packed file holds its streams in frames of 4 2-bit fields, or for
    I/Q, where 3 antennas take 6 fields, of 8 4-bit fields.  block: weights per block of ARRAY_BLOCK_FRAMES frames."""
    fs, f0 = (IQ_FILE_DECIMATED if D else IQ_FILE) if iq else REAL_FILE
    if first == "packed" and "frame" not in kw:
        kw.update(dict(bits=4, frame=8) if iq else dict(bits=2, frame=4))
    kw.setdefault("array_target_rms", ARRAY_TARGET_RMS[first])
    if block:
        kw["array_block_ms"] = 1000.0 * ARRAY_BLOCK_FRAMES / fs
    return Chain(first=first, dtype=dtype, D=MATRIX_D if D else 0, iq=iq, resamp=MATRIX_RESAMP if resamp else None, fs=fs,
                 f0=f0, antennas=antennas, **kw)


def array_matrix():
    """First stage x decimation x iqRecord x resampleUp at 3 antennas, whole-record weights, in a fixed order: 24 chains."""
    return [array_chain(first, dtype, D, iq, res) for first, dtype in ARRAY_FIRST_STAGES for D in (False, True)
            for iq in (False, True) for res in (False, True)]


# the variants: one chain each
ARRAY_BLOCK_REAL = array_chain("none", "int8", True, False, True, block=True)              # int8-a3b-d2-r5_3
ARRAY_BLOCK_IQ = array_chain("none", "uint8", False, True, False, block=True)              # uint8-a3b-iq
ARRAY_HOLD = array_chain("none", "uint8", True, False, False, block=True,                  # uint8-a3b-d2, a stretch of zeros
                         array_target_rms=ARRAY_TARGET_RMS["hold"])
ARRAY_ZERO_BLOCKS = {ARRAY_HOLD.name: (10, 15)}     # blocks 10 .. 14 of its file are zero: with W = 3 the windows of
ARRAY_HOLD_HELD = 3                                 # 11, 12 and 13 hold nothing
ARRAY_EIGHT = array_chain("none", "int8", False, True, False, antennas=8, array_taps=1)    # int8-a8k1-iq: 16-byte frames
ARRAY_TWO = array_chain("none", "int8", False, False, False, antennas=2, array_taps=15, array_reference=1)
ARRAY_PACKED_BYTES = array_chain("packed", "int8", False, False, False, frame=1, bits=2)   # packed2-a3: 4 samples a byte
ARRAY_NOTCH = array_chain("none", "int8", True, False, False, notch=True)                  # int8-a3-d2-notch
ARRAY_MONITOR = array_chain("none", "uint8", False, True, False, notch=True)               # uint8-a3-iq-notch, notchWholeRecord
ARRAY_MONITOR_SETTINGS = dict(notchWholeRecord=True, monitorSliceMs=2.5, monitorSegment=4096, monitorOverlap=1024)
# (four slices in the ten code periods the monitor sees, six segments each: the largest of a few single periodograms would
# cross the threshold somewhere by chance, and in segments much shorter the line does not stand 9 dB over the floor)
ARRAY_VARIANTS = (ARRAY_BLOCK_REAL, ARRAY_BLOCK_IQ, ARRAY_HOLD, ARRAY_EIGHT, ARRAY_TWO, ARRAY_PACKED_BYTES)
ARRAY_NOTCHES = (ARRAY_NOTCH, ARRAY_MONITOR)


def array_file_of(chain, native):
    """The file of a multi-antenna chain of the tables above, as tests/test_chain_array_gpu.py writes it."""
    return full_scale_file(chain, np.random.default_rng(ARRAY_SEED), file_components(chain, prepared_size(chain, native)))


# ---- sizes ------------------------------------------------------------------------------------------------------------------
PAD = 37                     # bytes beyond the two tile seams


def largest_tile(chain, native):
    """The most output one workgroup of a stage of this chain makes, in samples of that stage's output (native: the
    package's _native, whose *_tile() getters need no GPU)."""
    n = native
    tiles = [dict(packed=n.unpack_tile(), cond=n.cond_tile() * chain.lanes, requant=n.requant_tile()).get(chain.first, 0)]
    if chain.antennas:
        tiles.append(n.combine_tile())
    if chain.D:
        tiles.append(n.decim_tile())
    if chain.iq:
        tiles.append(n.iq_tile())
    if chain.resamp:
        tiles.append(n.resamp_tile() * chain.resamp[0] // 16)
    return max(tiles)


def smallest_offset(chain):
    """The smallest legal non-zero offset of the prepared record, found by asking file_range() about every one."""
    for offset in range(1, 4096):
        try:
            file_range(chain, offset, 2)
        except ValueError:
            continue
        return offset
    raise AssertionError(chain.name)


def prepared_size(chain, native):
    """The smallest prepared record that holds two tile seams of the largest tile and 37 bytes, and ten code periods (the
    window of the notch and of the probe) behind the smallest offset."""
    spc = prepared_settings(chain)["samplesPerCode"]
    return max(2 * largest_tile(chain, native) + PAD, 10 * spc + 2 * smallest_offset(chain))


# ---- a file with a line, for the chains that end in the notch ------------------------------------------------------------
LINE_OFFSET_HZ = 180e3           # the line stands about this far above the carrier in the prepared record ...
PROBE_BINS = 16384               # ... exactly on a bin of the probe's 16384-point spectrum: a periodic Hamming window leaks
                                 # an on-bin line into its two neighbours and no further
LINE_NOISE = 64                  # the noise is uniform in +-LINE_NOISE (rms 37) ...
LINE_AMPLITUDE = 12.0            # ... and the line a third of its rms: some 25 dB above the floor of the spectrum, its
                                 # harmonics behind a 2-bit quantiser far below it


LINE_SEED = 0xC4A2               # picked on the CPU so that notch_contract()'s precondition holds for every chain of the
                                 # matrix (tests/test_chain_host.py asserts it): a conditioned I/Q record keeps a trace of
                                 # its DC a quarter of the rate up, which some seeds put within 1 dB of the threshold


def notch_contract(chain, composed, at, threshold_db, width_hz, n_taps):
    """(lines, taps) of the notch behind the composed record (prepare()'s result): notch_spec.detect on the oracle's
    spectrum of the ten code periods from sample `at`, notch_spec.design for them.  The input must be well conditioned: no
    bin within 1 dB of the threshold - the GPU's spectrum, a few ulp from the oracle's, then flags the same bins - and the
    one line found is line_frequency()'s."""
    x = composed["record"]
    spc = samples_per_code(composed["fs"])
    assert x.size >= at + 10 * spc
    o = orc.OracleSettings(samplingFreq=composed["fs"], IF=composed["IF"])
    f, pxx, _ = orc.probe_stats(o, x[at:at + 10 * spc])
    with np.errstate(divide="ignore"):
        excess_db = 10.0 * np.log10(pxx / notch_spec.baseline(pxx))
    assert np.min(np.abs(excess_db - threshold_db)) > 1.0, (chain.name, float(np.min(np.abs(excess_db - threshold_db))))
    lines = notch_spec.detect(f, pxx, threshold_db, width_hz)
    f_line, _ = line_frequency(chain)
    assert len(lines) == 1 and abs(lines[0][0] - f_line) < 1.0, (chain.name, lines, f_line)
    return lines, notch_spec.design(lines, composed["fs"], n_taps)


def monitor_contract(chain, composed, at, threshold_db, width_hz, n_taps, slice_ms, segment, overlap):
    """(waterfall, lines, taps) of the notch with notchWholeRecord behind the composed record: waterfall_spec.waterfall of
    the record from sample `at` to its end, notch_spec.detect on its max-hold spectrum, notch_spec.design.  The same
    conditions as notch_contract: no bin within 1 dB of the threshold, and one line, whose notch covers line_frequency()'s
    (the monitor's segments are shorter than the probe's: the line stands on no bin of theirs)."""
    x, fs = composed["record"], composed["fs"]
    w = waterfall_spec.waterfall(x, at, x.size - at, fs / 1e6, int(segment), int(overlap), int(np.rint(slice_ms * 1e-3 * fs)))
    pxx = w["hold"]
    with np.errstate(divide="ignore"):
        excess_db = 10.0 * np.log10(pxx / notch_spec.baseline(pxx))
    assert np.min(np.abs(excess_db - threshold_db)) > 1.0, (chain.name, float(np.min(np.abs(excess_db - threshold_db))))
    lines = notch_spec.detect(w["f"], pxx, threshold_db, width_hz)
    f_line, _ = line_frequency(chain)
    assert len(lines) == 1 and abs(lines[0][0] - f_line) < lines[0][1] / 2.0, (chain.name, lines, f_line)
    return w, lines, notch_spec.design(lines, fs, n_taps)


def line_frequency(chain):
    """(frequency in the prepared record, frequency in the file's own terms) of the line, Hz."""
    r = rates(chain)
    df = r["fs"] / PROBE_BINS
    f_p = round((r["IF"] + LINE_OFFSET_HZ) / df) * df
    off = f_p - r["IF"]
    if r["decim"] is not None and r["decim"][4]:
        off = -off                       # an inverted band
    return f_p, chain.f0 + off


def line_file(chain, rng, components):
    """The bytes of a file of `components` components (packed: fields): uniform noise, the line of line_frequency(), both
    rails at known places."""
    n = int(components)
    _, f = line_frequency(chain)
    if chain.first == "packed" and chain.frame > 1:
        raise ValueError("one stream only")
    t = np.arange(n // chain.lanes, dtype=np.float64) / chain.fs
    v = rng.integers(-LINE_NOISE, LINE_NOISE + 1, n).astype(np.float64)
    arg = 2.0 * np.pi * f * t
    if chain.iq:
        i, q = (1, 0) if chain.q_first else (0, 1)
        v[i::2] += LINE_AMPLITUDE * np.cos(arg)
        v[q::2] += LINE_AMPLITUDE * np.sin(arg)
    else:
        v += LINE_AMPLITUDE * np.cos(arg)
    if chain.first == "packed":
        half = 1 << (chain.bits - 1)
        q = np.clip(np.floor(v / (2.0 * LINE_NOISE / (1 << chain.bits))), -half, half - 1).astype(np.int64)
        code = unpack_spec.code_of_level(chain.bits, unpack_spec.ENCODINGS[chain.encoding])[q + half]
        return unpack_spec.pack(code, chain.bits, unpack_spec.LSB_FIRST if chain.lsb_first else 0)
    x = np.clip(np.rint(v), -128, 127).astype(np.int8)
    x[::9973], x[5::9967] = -128, 127
    dt = np.dtype(chain.dtype)
    if dt == np.dtype(np.int8):
        return x.view(np.uint8)
    if dt == np.dtype(np.uint8):
        return x.view(np.uint8) ^ np.uint8(0x80)
    if dt == np.dtype(np.int16):
        return (x.astype("<i2") * 256).view(np.uint8)
    return (x.astype(np.float32) * np.float32(3.4e-5)).astype("<f4").view(np.uint8)
