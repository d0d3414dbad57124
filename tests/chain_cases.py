"""The composed contract of the record front end: what Settings._prepared_record(path, offset, count) must yield for a
chain of stages, built only from the numpy contracts of the single stages (tests/unpack_spec.py | cond_spec.py |
requant_spec.py -> decim_spec.py -> iq_spec.py -> resamp_spec.py), each designed by its own spec at the rate and IF the
contract in front of it produced.  The map from (offset, count) to the bytes of the file is written here from what the
stages say about themselves - which sample of an output is which sample of its input - and walks from the prepared record
back to the file, stage by stage.  The unit is the slice that is uploaded: a prepared record at an offset is the preparation
of that slice (filters start on zeros, the converter's quarter-rate carrier starts over), not a slice of the whole file's
prepared record.  numpy and the oracle only: no GPU, no package import.  Shared by tests/test_chain_host.py and tests/test_chain_gpu.py.
Test infrastructure, not product code."""
import numpy as np

import cond_spec
import notch_spec
import decim_spec
import iq_spec
import requant_spec
import resamp_spec
import unpack_spec
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
    that sees it."""

    def __init__(self, first="none", dtype="int8", D=0, iq=False, q_first=False, resamp=None, fs=16368000.0, f0=2000000.0,
                 bits=2, encoding="sign-magnitude", lsb_first=False, frame=1, first_field=0, peak=unpack_spec.DEFAULT_PEAK,
                 iq_taps=iq_spec.DEFAULT_TAPS, decim_taps=decim_spec.DEFAULT_TAPS, decim_bandwidth=decim_spec.DEFAULT_BANDWIDTH,
                 decim_gain=0.0, resamp_taps=0, resamp_cutoff=0.0, resamp_gain=1.0, cond_block_us=100.0, cond_agc_blocks=32.0,
                 cond_blank_factor=4.0, cond_guard=8, cond_target_rms=12.0, requant_target_rms=requant_spec.DEFAULT_TARGET_RMS,
                 notch=False):
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

    @property
    def name(self):
        first = {"none": self.dtype if self.dtype != "int8" else "none", "packed": "packed%d" % self.bits,
                 "cond": "cond_" + self.dtype, "requant": "requant_" + self.dtype}[self.first]
        if self.first == "packed" and self.frame > 1:
            first += "_f%d_%d" % (self.frame, self.first_field)
        parts = [first, "d%d" % self.D if self.D else None, ("qi" if self.q_first else "iq") if self.iq else None,
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
        for k, v in kw.items():
            setattr(s, k, v)
        return s


# ---- what each stage makes of the format: refusals as ValueError ----------------------------------------------------------

def _first_stage(chain):
    """(w, per_unit, unit): the first stage reads the file in units of `unit` bytes - the smallest run of whole bytes that
    holds whole elements (packed: whole frames) - and makes `per_unit` int8 components of each; w: bytes per component of an
    unpacked file.  Raises ValueError for a first stage that does not read this file."""
    dt = np.dtype(chain.dtype)
    if chain.first == "packed":
        if dt != np.dtype(np.int8):
            raise ValueError("a packed file is described as int8")
        take = 2 if (chain.iq and chain.frame > 1) else 1
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
    if dt == np.dtype(np.uint8) and chain.iq:
        return 1, 1, 1                                   # offset binary: the decimator or the converter takes it
    if dt != np.dtype(np.int8):
        raise ValueError("no stage of this chain reads %s" % dt.name)
    return 1, 1, 1


def _offset_binary_behind_first(chain):
    """Whether the int8 record behind the first stage still is offset binary: only where no stage has touched the file."""
    return chain.first == "none" and chain.dtype == "uint8"


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
    first stage, whole pairs, whole groups of D frames and whole groups of M samples in front of the resampler at once."""
    w, per_unit, unit = _first_stage(chain)
    need = chain.lanes * (chain.D or 1)                  # components: a group of D frames
    if chain.resamp:
        need = np.lcm(need, chain.resamp[1] * (chain.D or 1))   # ... M samples behind the decimator are M D in front of it
    units = int(np.lcm(int(need), per_unit)) // per_unit
    return units * unit


def prepared_skip(chain, skip_bytes):
    """The sample of the prepared record that byte skip_bytes of the file becomes, walking forwards; ValueError where the
    byte does not begin a sample of every record along the chain."""
    w, per_unit, unit = _first_stage(chain)
    skip_bytes = int(skip_bytes)
    if skip_bytes % unit:
        raise ValueError("the byte splits %s" % ("a frame" if chain.first == "packed" else "a component"))
    pos = skip_bytes // unit * per_unit                  # component of the int8 record behind the first stage
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
    if start % per_unit:
        raise ValueError("sample %d does not start a frame of the packed file" % start)
    first = start // per_unit * unit
    units = (n + per_unit - 1) // per_unit               # whole units: a packed file is read frame by frame
    return first, units * unit


def components_per_unit(chain):
    """(components the first stage makes of one unit of the file, bytes of that unit)."""
    _, per_unit, unit = _first_stage(chain)
    return per_unit, unit


def prepared_length(chain, n_bytes):
    """Samples of the prepared record of a file of n_bytes bytes (whole units), walking forwards."""
    w, per_unit, unit = _first_stage(chain)
    n = int(n_bytes) // unit * per_unit
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
    if chain.D:
        extra = chain.lanes * -(-(-(-extra // chain.lanes)) // chain.D)
    if chain.resamp:
        L, M = chain.resamp
        extra = -(-(extra + 1 + (1 if chain.iq else 0)) * L // M)
    return max(extra, chain.lanes - 1)                   # (an odd count in front of the converter: a whole pair)


# ---- the composition --------------------------------------------------------------------------------------------------

def prepare(file_bytes, chain, offset, count, requant_sums=None):
    """What _prepared_record(path, offset, count) must yield for a file holding file_bytes: dict with `record` (int8), per
    stage that ran a dict of the contract's counts - unpack (samples, code_counts), cond (samples, block, blocks, blanked
    frames, clipped), requant (samples, clipped, mult, shift, scale), decim (samples, clipped, fs_out, f_out, inverted),
    resamp (samples, clipped, fs_out) - and the prepared (fs, IF).  A file that ends inside the range is read as far as it
    goes; of a packed file whole frames are kept; any other file must then end on whole elements and pairs (ValueError from
    the stage's contract otherwise).  requant_sums: (n_finite, sum_sq) as the library summed a float32 file, which its
    contract lets differ from the correctly rounded sums by requant_spec.bounds(); None: the contract's own."""
    raw = np.ascontiguousarray(file_bytes).view(np.uint8).ravel()
    w, per_unit, unit = _first_stage(chain)
    r = rates(chain)
    first, n_bytes = file_range(chain, offset, count)
    b = raw[first:first + n_bytes]
    out = dict(fs=r["fs"], IF=r["IF"], file_range=(first, b.size))
    if chain.first == "packed":
        b = b[:b.size // unit * unit]                    # a frame the file ends in is left
        out["file_range"] = (first, b.size)
        take = 2 if (chain.iq and chain.frame > 1) else 1
        table = unpack_spec.table(chain.bits, unpack_spec.ENCODINGS[chain.encoding], chain.peak)
        flags = unpack_spec.LSB_FIRST if chain.lsb_first else 0
        x = unpack_spec.unpack(b, chain.bits, table, flags, chain.frame, chain.first_field, take)
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
    ob = _offset_binary_behind_first(chain)
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
    full-scale values at 3.4e-5 of their size."""
    n = int(components)
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


# ---- sizes ------------------------------------------------------------------------------------------------------------------
PAD = 37                     # bytes beyond the two tile seams


def largest_tile(chain, native):
    """The most output one workgroup of a stage of this chain makes, in samples of that stage's output (native: the
    package's _native, whose *_tile() getters need no GPU)."""
    n = native
    tiles = [dict(packed=n.unpack_tile(), cond=n.cond_tile() * chain.lanes, requant=n.requant_tile()).get(chain.first, 0)]
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
