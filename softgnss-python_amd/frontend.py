"""The record front end of Settings: the stages that stand between a record file and acquisition.

STAGES is the one ordered table: unpack -> combine | condition | requantise -> decimate -> convert -> resample (the swept-interference
excision and the notch follow them and change no position); what an entry says of its stage is listed at _Stage.  FrontEnd._walk folds the table forwards over
the file's settings, _file_range walks the same pairs backwards and _prepared_record runs the stages in one loop: the shape
of the composed contract, tests/chain_cases.py.  main.py builds its command line and its banner from the same table.
"""
import contextlib
import copy
import os

import numpy as np

from . import _native


def _with(s, **changes):
    """A copy of the settings s with the attributes `changes`."""
    out = copy.copy(s)
    out.__dict__.update(changes)
    return out


class _Stage(object):
    """An entry of STAGES.  name; flag: the setting that switches the stage on; defaults: its settings; last: the attribute
    of the file's settings that keeps run()'s info; reads / makes: what n_in positions of its input and n_out of its output
    are, for the refusals.  step(s) -> (n_in, n_out, out), under the settings s the stage reads under: the format check, the
    design and the position rule - positions of the record it reads are legal on multiples of n_in, and n_in of them become
    n_out of the record it writes - and the settings its output is read under (the walk maps skipNumberOfBytes).
    run(s, raw, say, prepared) -> (record, info) through the public method, between the two lines `say` prints.
    The command line: options: (flag, add_argument's keywords), first the one that switches the stage on; usage: its
    paragraph of main's docstring; needs: the refusal of the others without the first; settings_from(args, fail), where the
    first is given -> the settings asked for (None: left alone), by the options' own syntax and the checks _walk() does not
    make - fail(message) does not return; replays_file: --correlator-bank can replay from the file behind it (else verb:
    what it does to its positions); announce(file): its line of the banner, which main.py ends with the prepared rate and IF."""
    last = needs = announce = None
    replays_file = True

    def on(self, s):
        return bool(getattr(s, self.flag))

    def count_in(self, file, count, n_in, n_out):    # positions of its input that `count` of its output are made of
        return -(-count * n_in // n_out)


def _numbers(text, seps):
    """[A, B, C] of an option's text 'A[/B][:C]' (seps '/:'; None for a part that is left out), or None for any other text."""
    out = []
    try:
        for sep in reversed(seps):                   # the last part first: '7/3:127' -> '7/3', 127 -> '7', 3, 127
            text, found, tail = text.partition(sep)
            out.insert(0, int(tail) if found else None)
        return [int(text)] + out
    except ValueError:
        return None


# 1-, 2- and 4-bit packed records (Settings.unpackRecord; INTEGRATION.md, "Packed records"): the file is unpacked to one int8
# sample per selected field on the GPU, first of all stages
class _Unpack(_Stage):
    name, flag, last = "unpack", "packedBits", "lastUnpack"
    reads, makes = "a frame of the packed file", "the samples of a frame of the packed file"
    defaults = (
        ("packedBits", 0),                   # bits per sample of the file: 1, 2 or 4; 0: the stage is off
        ("packedEncoding", 'sign-magnitude'),   # or 'offset-binary', 'twos-complement': what a code means
        ("packedLsbFirst", False),           # the first sample of a byte lies in its low bits
        ("packedFrame", 1),                  # F: fields per frame (1, 2, 4, 8 or 16) of a file that interleaves several streams
        ("packedFirst", 0),                  # the field of a frame the selection starts at
        ("packedPeak", 48),                  # the largest level of the int8 record it makes, LSB, in 2^bits - 1 .. 127
        ("packedTable", None),               # an explicit sequence of 2^bits int8 levels, one per code: overrides encoding and peak
    )
    options = (("--packed", dict(type=int, default=None, choices=(1, 2, 4), metavar="BITS",
                    help="the file holds packed BITS-bit samples (1, 2 or 4): unpack it to int8 on the GPU before anything "
                         "else")),
               ("--packed-encoding", dict(default=None, choices=("sign-magnitude", "offset-binary", "twos-complement"),
                    help="with --packed: what a code means (default: Settings.packedEncoding, sign-magnitude)")),
               ("--packed-lsb-first", dict(action="store_true",
                    help="with --packed: the first sample of a byte lies in its low bits")),
               ("--packed-frame", dict(default=None, metavar="F[:FIRST]",
                    help="with --packed: the file interleaves streams in frames of F fields (1, 2, 4, 8 or 16); keep the "
                         "field at FIRST (default 0; with --iq the I/Q pair from there on)")),
               ("--packed-peak", dict(type=int, default=None, metavar="PEAK",
                    help="with --packed: the largest level of the int8 record (default: Settings.packedPeak, 48)")))
    needs = "--packed-encoding, --packed-lsb-first, --packed-frame and --packed-peak describe a packed file: they need --packed"
    usage = """--packed BITS (1, 2 or 4; real or with --iq) reads a file of packed samples: the GPU unpacks it first of all into
one int8 sample per field, through the levels of --packed-encoding (sign-magnitude, offset-binary or twos-complement) scaled to
--packed-peak (48), the first sample of a byte in its high bits (--packed-lsb-first: in its low bits), and prints the share of the
samples on each level.  --packed-frame F[:FIRST] is for files that interleave several streams: of every F fields (2, 4, 8 or 16)
the one at FIRST is kept (with --iq the pair from FIRST on).  --skip stays a byte of the file, on a frame boundary; positions in
the results are samples of the unpacked record.  Not with --iq-requantize or --condition."""

    def settings_from(self, args, fail):
        frame, first = _numbers("1" if args.packed_frame is None else args.packed_frame, ":") or \
            fail("--packed-frame takes F[:FIRST] with F one of 1, 2, 4, 8, 16 and the kept fields inside the frame")
        return dict(packedBits=args.packed, packedEncoding=args.packed_encoding, packedLsbFirst=args.packed_lsb_first or None,
                    packedFrame=frame, packedFirst=first or 0, packedPeak=args.packed_peak)

    def step(self, s):
        unit, samples = s._pack_units()
        return unit, samples, _with(s, packedBits=0)

    def whole(self, file, n_in, n_out):
        """(bytes of the file, samples of the unpacked record) of the least run that holds whole frames of the packed file
        and, with Settings.antennas, whole frames of all antennas: where the samples of a byte are not whole antenna
        frames (packedFrame = 1: 2-bit samples of 3 antennas) the least common multiple of the two."""
        if not _Combine().on(file):
            return n_in, n_out
        lanes, A = file._array_format()[:2]
        k = int(np.lcm(n_out, A * lanes)) // n_out
        return k * n_in, k * n_out

    def count_in(self, file, count, n_in, n_out):
        n_in, n_out = self.whole(file, n_in, n_out)
        return -(-count // n_out) * n_in             # whole frames (with iqRecord n_out is even: whole pairs)

    def run(self, s, raw, say, prepared):
        say('   Unpacking %d-bit samples to int8...' % int(s.packedBits))
        rec, info = s.unpackRecord(raw)
        say('   %d samples; levels %s' % (info["samples"], ", ".join(
            "%+d: %.2f %%" % (int(lv), 100.0 * sh) for lv, sh in sorted(zip(info["table"], info["shares"])))))
        return rec, info


# multi-antenna records (Settings.combineAntennas; INTEGRATION.md, "Multi-antenna records"): the streams of several antennas go
# through a space-time combiner whose power-inversion weights cancel what stands above the noise - a broadband jammer - and
# come out as one int8 record, directly behind the unpacker
class _Combine(_Stage):
    name, flag, last = "combine", "antennas", "lastCombining"
    reads, makes = "a frame of all antennas", "a frame"
    defaults = (
        ("antennas", 0),                     # A: the file interleaves that many streams, 2 .. 8; 0: the stage is off
        ("arrayTaps", 0),                    # K: taps per antenna (odd, at most 15, A K <= 64); 0: 1 for iqRecord, 5 for a real record
        ("arrayReference", 0),               # the antenna whose centre tap is held at 1
        ("arrayLoading", 1e-3),              # diagonal loading, in units of the mean power of the streams
        ("arrayTargetRms", 12.0),            # rms of the int8 record it makes, LSB, in (0, 127]
        ("arrayBlockMs", 0),                 # weights per block of about that many ms (whole multiples of 4096 frames); 0: one set per record
        ("arrayWindowBlocks", 3),            # a block's weights come from the statistics of that many blocks around it (odd, 1 .. 63)
    )
    options = (("--antennas", dict(default=None, metavar="A[:REF]",
                    help="the file interleaves the streams of A antennas (2 .. 8), frame by frame: combine them on the GPU "
                         "into one record with power-inversion weights that null a jammer, antenna REF (default 0) held at 1")),
               ("--array-taps", dict(type=int, default=None, metavar="K",
                    help="with --antennas: taps per antenna (odd, 1 .. 15, A x K <= 64; default: 1 with --iq, else 5)")),
               ("--array-block", dict(default=None, metavar="MS[:WINDOW]",
                    help="with --antennas: new weights every MS ms (to a whole multiple of 4096 frames), each set from the "
                         "statistics of WINDOW blocks around its own (odd, 1 .. 63; default 3): follows a jammer or an "
                         "antenna that moves")))
    needs = "--array-taps and --array-block describe the antenna combiner: they need --antennas"
    replays_file, verb = False, "combines"
    usage = """--antennas A[:REF] (A = 2 .. 8; int8 or uint8 files, real or with --iq, or the A streams of a --packed file) reads a
file that interleaves the streams of A antennas frame by frame: the GPU takes the exact cross-correlations of the streams,
the host designs power-inversion weights from them - least output power with antenna REF (0) held at 1, which nulls a
broadband jammer and needs no array geometry - and the GPU runs every stream through a --array-taps K tap integer FIR (1 with
--iq, else 5) and sums them into one int8 record at 12 LSB rms, in front of every other stage.  The suppression of the
reference antenna's power, the largest weight and the share of clipped samples are printed.  --array-block MS[:WINDOW]
designs new weights for every block of MS ms (a whole multiple of 4096 frames) from the statistics of WINDOW blocks around it
(3), for a jammer or an antenna that moves; the least and the median suppression over the blocks are printed.  --skip stays a
byte of the file, on a frame of all antennas; positions in the results are samples of the combined record.  Not with
--condition or --iq-requantize."""

    def settings_from(self, args, fail):
        A, ref = _numbers(args.antennas, ":") or (0, None)
        if not A:                            # (A = 0 is Settings.antennas' word for "the stage is off")
            fail("--antennas takes A[:REF] with A in 2 .. 8 and REF one of the antennas 0 .. A - 1")
        if args.array_taps is not None and args.array_taps <= 0:     # (0 is Settings' word for "the default length")
            fail("--array-taps takes the taps per antenna, odd, 1 .. 15")
        block_ms = window = None
        if args.array_block is not None:
            ms, found, tail = args.array_block.partition(":")
            try:
                block_ms, window = float(ms), int(tail) if found else None
            except ValueError:
                block_ms = None
            if block_ms is None or not (np.isfinite(block_ms) and block_ms > 0):     # (0 is Settings' word for "one set per record")
                fail("--array-block takes MS[:WINDOW] with the block length MS in ms, above 0, and WINDOW blocks, odd, 1 .. 63")
        return dict(antennas=A, arrayReference=ref, arrayTaps=args.array_taps, arrayBlockMs=block_ms, arrayWindowBlocks=window)

    def announce(self, file):
        return 'Combined %d antennas' % file.antennas

    def step(self, s):
        lanes, A = s._array_format()[:2]
        return A * lanes, lanes, _with(s, antennas=0, dataType='int8')

    def run(self, s, raw, say, prepared):
        lanes, A, K = s._array_format()[:3]
        say('   Combining %d antennas through %d tap%s each...' % (A, K, "" if K == 1 else "s"))
        rec, info = s.combineAntennas(raw)
        if "blocks" in info:
            say('   %d samples in %d blocks of %d frames (%d held): reference antenna suppressed by %.2f dB at the least, %.2f dB '
                'in the median, largest |weight| %.3f, median gain %+.2f dB, %.4f %% of the samples clipped'
                % (info["samples"], info["blocks"], info["block_frames"], info["held_blocks"], info["suppression_db_min"],
                   info["suppression_db"], float(np.max(np.abs(info["weights"]))), info["gain_db"], 100.0 * info["clipped"]))
            return rec, info
        say('   %d samples: reference antenna suppressed by %.2f dB, largest |weight| %.3f, gain %+.2f dB, %.4f %% of the '
            'samples clipped' % (info["samples"], info["suppression_db"], float(np.max(np.abs(info["weights"]))),
                                 info["gain_db"], 100.0 * info["clipped"]))
        return rec, info


# block-wise front-end conditioning (Settings.conditionRecord; INTEGRATION.md, "Front-end conditioning"): DC removal, a
# time-varying AGC and pulse blanking per short block, first of all stages, where the fixed-gain requantiser sits otherwise
class _Condition(_Stage):
    name, flag, last = "condition", "frontEndConditioning", "lastConditioning"
    reads = makes = "a sample"
    defaults = (
        ("frontEndConditioning", False),     # the stage is off
        ("condBlockUs", 100.0),              # block length: that many frames at samplingFreq, to a multiple of 16 in 256 .. 16384
        ("condAgcBlocks", 32.0),             # the AGC's smoothing length in blocks
        ("condBlankFactor", 4.0),            # c: a frame beyond c x the smoothed rms is blanked; blank_q4 = rint(16 c^2); 0: off
        ("condGuardFrames", 8),              # frames blanked either side of a hit
        ("condTargetRms", 12.0),             # rms of the int8 record it makes, LSB, in (0, 127]
    )
    options = (("--condition", dict(nargs="?", type=float, const=-1.0, default=None, metavar="BLANK_FACTOR",
                    help="condition the file block by block on the GPU before anything else: DC removal, AGC and pulse "
                         "blanking at BLANK_FACTOR x the rms (default: Settings.condBlankFactor, 4; 0: no blanking)")),)
    usage = """--condition (--dtype int8, uint8 or int16, real or with --iq) first conditions the file block by block on the GPU:
per 100 us it removes the DC of each rail, sets the gain that puts the rms at 12 LSB (a time-varying AGC) and zeroes the frames
that stand 4 x (or --condition=BLANK_FACTOR, 1 .. 16; 0: no blanking) above the rms, and prints the span of the gain and the
shares of blanked frames and clipped samples; it stands where --iq-requantize does, so not both; an int16 file is then read as
int8, positions are file byte / 2."""

    def settings_from(self, args, fail):
        if not (args.condition in (-1.0, 0.0) or 1.0 <= args.condition <= 16.0):     # (-1: no value given, the default)
            fail("--condition takes the blanking threshold in units of the rms, 1 .. 16, or 0 for no blanking")
        return dict(frontEndConditioning=True, condBlankFactor=args.condition if args.condition >= 0 else None)

    def step(self, s):
        return s._cond_format()[0], 1, _with(s, frontEndConditioning=False, dataType='int8')

    def run(self, s, raw, say, prepared):
        say('   Conditioning %s samples block by block...' % np.dtype(s.dataType).name)
        rec, info = s.conditionRecord(raw)
        say('   %d blocks of %d frames: gain %+.2f .. %+.2f dB, %.4f %% of the frames blanked, %.4f %% of the '
            'samples clipped' % (info["blocks"], info["block"], info["gain_db_min"], info["gain_db_max"],
                                 100.0 * info["blanked"], 100.0 * info["clipped"]))
        return rec, info


# int16 (sc16) and float32 (fc32) I/Q files (Settings.requantizeIQ; INTEGRATION.md, "int16 / float32 I/Q"): the file is
# brought to int8 on the GPU through one fixed gain, ahead of the converter
class _Requantise(_Stage):
    name, flag, last = "requantise", "iqRequantize", "lastRequant"
    reads = makes = "a sample"
    defaults = (
        ("iqRequantize", False),             # with iqRecord: dataType 'int16' and 'float32' are read through the requantiser
        ("iqTargetRms", 12.0),               # rms of the int8 record it makes, LSB, in (0, 127]
    )
    options = (("--iq-requantize", dict(nargs="?", type=float, const=-1.0, default=None, metavar="RMS",
                    help="with --iq and --dtype int16 or float32: bring the file to int8 on the GPU through one fixed gain "
                         "that puts its rms at RMS LSB (default: Settings.iqTargetRms, 12)")),)
    usage = """--iq-requantize (with --iq and --dtype int16 or float32: sc16 and fc32 captures) first brings the file to int8 on
the GPU through one fixed gain that puts its rms at 12 LSB (or --iq-requantize=RMS), and prints the record's rms, peak, count of
non-finite samples, the gain in dB and the share of clipped samples; --skip stays a byte of the file (a multiple of 4 for int16, 8
for float32), the positions in the results are samples of the converted record, file byte / 2 or / 4."""

    def settings_from(self, args, fail):
        if args.iq is None:                 # (_walk() lets it pass: without iqRecord the setting switches nothing on)
            fail("--iq-requantize prepares an I/Q file for the converter: it needs --iq")
        if not (args.iq_requantize == -1.0 or 0.0 < args.iq_requantize <= 127.0):       # (-1: no value given, the default)
            fail("--iq-requantize takes the rms of the int8 record in LSB, above 0 and at most 127")
        return dict(iqRequantize=True, iqTargetRms=args.iq_requantize if args.iq_requantize > 0 else None)

    def on(self, s):                         # (without iqRecord the flag switches nothing on; an 8-bit file needs no gain)
        return bool(s.iqRecord and s.iqRequantize) and np.dtype(s.dataType).itemsize > 1

    def step(self, s):
        return s._iq_width(), 1, _with(s, iqRequantize=False, dataType='int8')

    def run(self, s, raw, say, prepared):
        say('   Requantising %s samples to int8...' % np.dtype(s.dataType).name)
        rec, info = s.requantizeIQ(raw)
        say('   rms %.6g, peak %.6g, %d non-finite samples, gain %+.2f dB, %.4f %% of the samples clipped'
            % (info["rms"], info["max_abs"], info["n_nonfinite"], info["gain_db"], 100.0 * info["clipped"]))
        return rec, info


# band selection and decimation ahead of acquisition (Settings.decimateRecord; INTEGRATION.md, "Decimation"): the int8 record
# goes through a band-pass around the carrier and comes out at 1 / decimation of the rate
class _Decimate(_Stage):
    name, flag, last = "decimate", "decimation", "lastDecimation"
    reads, makes = "a group of Settings.decimation frames", "a frame"
    defaults = (
        ("decimation", 0),                   # the factor D, 2 .. 16; 0: the stage is off
        ("decimTaps", 127),                  # filter length (odd, at most 511)
        ("decimBandwidth", 2.046e6),         # two-sided bandwidth of the band that is kept, Hz
        ("decimGain", 0.0),                  # 0: the gain that keeps a white input's rms
    )
    options = (("--decimate", dict(default=None, metavar="D[:TAPS]",
                    help="select the band around the carrier and decimate the record by D (2 .. 16) on the GPU, through a "
                         "band-pass of TAPS taps (odd, at most 511; default: Settings.decimTaps, 127)")),
               ("--decimate-bandwidth", dict(type=float, default=None, metavar="HZ",
                    help="with --decimate: the two-sided bandwidth that is kept (default: Settings.decimBandwidth, 2.046e6)")))
    needs = "--decimate-bandwidth describes the band --decimate keeps: it needs --decimate"
    replays_file, verb = False, "resamples"
    usage = """--decimate D[:TAPS] (D = 2 .. 16; real int8 records, or with --iq, --condition, --packed) selects the band
--decimate-bandwidth wide (2.046 MHz) around the carrier with a TAPS-tap band-pass (127) on the GPU and keeps every D-th sample,
behind the other preparing stages and in front of the I/Q converter and the notch: everything else runs at 1 / D of the rate.  The
new rate, where the carrier lands, whether the band came out inverted (the Doppler then shows with the other sign) and the share
of clipped samples are printed.  --skip stays a byte of the file, on a multiple of D frames; positions in the results are samples
of the prepared record, D input frames each.  A --fs / --IF pair whose band would alias onto itself at this D is refused (the
default record at D = 2 or 4: use 3 or 5)."""

    def settings_from(self, args, fail):
        D, taps = _numbers(args.decimate, ":") or (0, None)
        if not D:                            # (D = 0 is Settings.decimation's word for "the stage is off")
            fail("--decimate takes D[:TAPS] with D in 2 .. 16 and TAPS odd, 1 .. 511")
        bandwidth = args.decimate_bandwidth
        if bandwidth is not None and not (np.isfinite(bandwidth) and bandwidth > 0):
            fail("--decimate-bandwidth takes the two-sided bandwidth in Hz, above 0")
        return dict(decimation=D, decimTaps=taps, decimBandwidth=bandwidth)

    def announce(self, file):
        return 'Decimated by %d' % file.decimation

    def step(self, s):
        lanes, D = s._decim_format()[:2]
        info = s._decim_design()[2]
        return lanes * D, lanes, _with(s, decimation=0, dataType='int8', samplingFreq=info["fs_out"], IF=info["f_out"])

    def run(self, s, raw, say, prepared):
        say('   Decimating by %d through %d taps...' % (int(s.decimation), int(s.decimTaps)))
        rec, info = s.decimateRecord(raw)
        say('   %d samples at %.6g Msps, %s %.6g MHz, band %s, %.4f %% of the samples clipped'
            % (info["samples"], info["fs_out"] / 1e6, "carrier at" if s.iqRecord else "IF", info["f_out"] / 1e6,
               "INVERTED (Doppler shows with the other sign)" if info["inverted"] else "upright", 100.0 * info["clipped"]))
        return rec, info


# interleaved 8-bit I/Q baseband records (Settings.convertIQ; INTEGRATION.md, "I/Q baseband records"): the record is turned
# into the equivalent real IF record on the GPU and every later stage runs on that, under Settings.realEquivalent().  Byte n
# of the converted record is the instant of byte n's pair: an upload from an odd one would start on a Q, read as I from there on
class _Convert(_Stage):
    name, flag = "convert", "iqRecord"
    reads = makes = "an I/Q pair (Settings.iqRecord)"
    defaults = (
        ("iqRecord", False),                 # fileName holds interleaved I/Q: samplingFreq is the COMPLEX rate, IF the baseband
                                             # offset (0 or negative allowed), dataType 'int8' or 'uint8' (offset binary)
        ("iqQFirst", False),                 # the file holds Q before I (also: spectral inversion of an I-first file)
        ("iqTaps", 63),                      # length of the interpolation filter (odd, at most 255)
    )
    options = (("--iq", dict(nargs="?", const="iq", default=None, choices=("iq", "qi"), metavar="qi",
                    help="the file is interleaved 8-bit I/Q (--iq=qi: Q first): --fs is the complex rate, --IF the "
                         "baseband offset; it is converted to real IF at twice the rate on the GPU")),)
    replays_file, verb = False, "converts"
    usage = """--iq reads the file as interleaved 8-bit I/Q (--iq=qi: Q before I; --dtype uint8: offset binary, as an RTL-SDR
writes it): --fs is then the COMPLEX rate and --IF the baseband offset of the carrier (0 for a zero-IF front end); the GPU turns
the file into the equivalent real record at twice the rate, whose rate and IF are printed, and everything else runs on that."""

    def settings_from(self, args, fail):
        return dict(iqRecord=True, iqQFirst=args.iq == "qi" or None)

    def announce(self, file):
        return 'I/Q record at %.6f Msps, carrier at %+.6f MHz' % (file.samplingFreq / 1e6, file.IF / 1e6)

    def step(self, s):
        s._iq_format()
        return 2, 2, s.realEquivalent()

    def run(self, s, raw, say, prepared):
        # (the rate and IF named are the prepared record's: behind a resampler, the resampled rate)
        say('   Converting I/Q at %.6g Msps to real IF: %.6g Msps, IF %.6g MHz...'
            % (s.samplingFreq / 1e6, prepared.samplingFreq / 1e6, prepared.IF / 1e6))
        return s.convertIQ(raw), None


# rational resampling ahead of acquisition (Settings.resampleRecord; INTEGRATION.md, "Resampling"): the real int8 record goes
# through a polyphase low-pass and comes out at resampleUp / resampleDown of the rate - a capture below the 15.4 samples per
# chip the fast tracking kernels need reaches them
class _Resample(_Stage):
    name, flag, last = "resample", "resampleUp", "lastResampling"
    reads, makes = "a group of Settings.resampleDown samples", "a group of Settings.resampleUp samples"
    defaults = (
        ("resampleUp", 0),                   # the up factor L, 2 .. 16; 0: the stage is off
        ("resampleDown", 1),                 # the down factor M, 1 .. 3, below L and coprime to it
        ("resampTaps", 0),                   # filter length at the stuffed rate (odd, at most 1023); 0: 24 L + 1
        ("resampCutoff", 0.0),               # cutoff of the low-pass, Hz; 0: half the lower of the two rates
        ("resampGain", 1.0),
    )
    options = (("--resample", dict(default=None, metavar="L[/M][:TAPS]",
                    help="bring the real int8 record to L / M of its rate on the GPU (L 2 .. 16, M 1 .. 3, M < L, coprime), "
                         "through a low-pass of TAPS taps (odd, at most 1023; default: 24 L + 1)")),
               ("--resample-cutoff", dict(type=float, default=None, metavar="HZ",
                    help="with --resample: the cutoff of the low-pass (default: half the lower of the two rates)")))
    needs = "--resample-cutoff describes the low-pass of --resample: it needs --resample"
    replays_file, verb = False, "resamples"
    usage = """--resample L[/M][:TAPS] (L = 2 .. 16, M = 1 .. 3 below L and coprime to it) brings the real int8 record - the
file, or what the stages above make of it - to L / M of its rate on the GPU through a TAPS-tap low-pass (24 L + 1) that cuts off
at --resample-cutoff (half the lower of the two rates), in front of the notch: a capture below the 15.4 samples per chip the fast
tracking kernels need reaches them (4.096 Msps: 10, 16.368 Msps: 7/3, 2.048 Msps I/Q: --iq with 10).  The new rate and the share
of clipped samples are printed.  --skip stays a byte of the file, on a sample that maps to a whole one (a multiple of M);
positions in the results are samples of the resampled record."""

    def settings_from(self, args, fail):
        (L, M, taps), cutoff = _numbers(args.resample, "/:") or (0, 0, 0), args.resample_cutoff
        if not L or taps == 0:               # (0 is Settings' word for "the stage is off" and for "the default length")
            fail("--resample takes L[/M][:TAPS] with L in 2 .. 16, M in 1 .. 3 below L and coprime to it, and TAPS odd, "
                 "1 .. 1023")
        if cutoff is not None and not (np.isfinite(cutoff) and cutoff > 0):
            fail("--resample-cutoff takes the cutoff in Hz, above 0")
        return dict(resampleUp=L, resampleDown=1 if M is None else M, resampTaps=taps, resampCutoff=cutoff)

    def announce(self, file):
        return 'Resampled by %d/%d' % (file.resampleUp, file.resampleDown)

    def step(self, s):
        L, M, _ = s._resamp_format()
        info = s._resamp_design()[2]
        return M, L, _with(s, resampleUp=0, samplingFreq=info["fs_out"])

    def count_in(self, file, count, n_in, n_out):
        count = -(-count * n_in // n_out)            # every input sample that starts inside the span of the outputs
        return count + count % 2 if _Convert().on(file) else count    # (a converter in front makes whole pairs)

    def run(self, s, raw, say, prepared):
        say('   Resampling by %d/%d through %d taps...' % s._resamp_format())
        rec, info = s.resampleRecord(raw)
        say('   %d samples at %.6g Msps, %.4f %% of the samples clipped'
            % (info["samples"], info["fs_out"] / 1e6, 100.0 * info["clipped"]))
        return rec, info


STAGES = (_Unpack(), _Combine(), _Condition(), _Requantise(), _Decimate(), _Convert(), _Resample())     # the order: written here only

# narrowband interference excision (Settings.mitigate; INTEGRATION.md, "Interference excision"): continuous-wave lines found
# in the Welch spectrum of probeData are notched out of the prepared record by a zero-phase integer FIR, behind all stages
_NOTCH_DEFAULTS = (
    ("interferenceMitigation", False),   # postProcessing() filters the record before acquisition and tracking
    ("notchThresholdDb", 8.0),           # a PSD bin this far above the running median of its neighbourhood is a line
    ("notchWidthHz", 80e3),              # least width of a notch
    ("notchTaps", 1025),                 # filter length (odd, at most 4095)
)

# swept (chirp) interference excision (Settings.excise; INTEGRATION.md, "Swept interference"): every short segment of the
# prepared record loses the bins that stand out of its own spectrum, directly in front of the notch
_EXCISE_DEFAULTS = (
    ("sweptMitigation", False),          # postProcessing() excises the record before the notch, acquisition and tracking
    ("exciseSegment", 256),              # segment length, a power of two in 64 .. 1024; the hop is half of it
    ("exciseThreshold", 8.0),            # a bin this many times the mean of the segment's kept bins is cut (at least 1)
    ("excisePasses", 3),                 # rounds of mean and cut, 1 .. 8
)

# the record monitor (Settings.monitorRecord; INTEGRATION.md, "Monitoring a record"): the spectrum and the sample statistics
# of the whole prepared record, slice by slice - what the notch is designed from where notchWholeRecord is set
_MONITOR_DEFAULTS = (
    ("monitorSliceMs", 100.0),           # slice length: one spectrum and one set of statistics per that many ms
    ("monitorSegment", 16384),           # Welch segment length, a power of two in 256 .. 16384
    ("monitorOverlap", 1024),            # samples two consecutive segments share
    ("monitorMinSlices", 2),             # a line seen in fewer consecutive slices is no event
    ("notchWholeRecord", False),         # mitigate() designs the notch from the monitor's max-hold spectrum
)
MONITOR_PULSED_MADS = 6.0                # a slice is pulsed beyond the median + this many scaled MADs of the record's slices

DEFAULTS = sum((stage.defaults for stage in STAGES), ()) + _EXCISE_DEFAULTS + _NOTCH_DEFAULTS + _MONITOR_DEFAULTS
# help of main's --dtype: no stage's own option, but which sample types a file may hold is what the stages above read
DTYPE_HELP = "dataType of the file's samples (numpy name; with --iq: int8 or uint8, with --iq-requantize also int16 or float32)"


def _multiple(n):
    return "even" if n == 2 else "a multiple of %d" % n


def line_peak_db(f_mhz, pxx, f_hz, width_hz):
    """How far a line stands above its floor, dB: the largest bin of the band [f_hz - width_hz / 2, f_hz + width_hz / 2]
    over the median of the 257 bins around it (the baseline notch_design flags against)."""
    f = np.asarray(f_mhz) * 1e6
    band = np.flatnonzero(np.abs(f - f_hz) <= width_hz / 2.0)
    if not band.size:
        band = np.array([int(np.argmin(np.abs(f - f_hz)))])
    k = int(band[np.argmax(pxx[band])])
    floor = float(np.median(pxx[max(0, k - 128):k + 129]))
    return float(10.0 * np.log10(pxx[k] / floor)) if floor > 0 and pxx[k] > 0 else float("inf")


def monitor_events(per_slice, slice_ms, min_slices):
    """The lines of the slices merged into events.  per_slice[j]: the lines (f_hz, width_hz, peak_db) of slice j in
    ascending frequency.  A line continues an event seen in slice j - 1 when their bands [f - w / 2, f + w / 2] overlap
    (the oldest such event), else it opens one.  An event's f_hz and peak_db are those of its strongest slice, its width
    the widest; first_ms = first slice x slice_ms, last_ms = (last slice + 1) x slice_ms.  Events of fewer than min_slices
    slices are dropped; the rest come in order of (first_ms, f_hz), each (f_hz, width_hz, first_ms, last_ms, peak_db)."""
    events = []
    for j, lines in enumerate(per_slice):
        for f, w, peak in lines:
            lo, hi = f - w / 2.0, f + w / 2.0
            for e in events:
                if e["last"] == j - 1 and lo <= e["hi"] and e["lo"] <= hi:
                    if peak > e["peak"]:
                        e["f"], e["peak"] = f, peak
                    e.update(w=max(e["w"], w), last=j, lo=lo, hi=hi)
                    break
            else:
                events.append(dict(f=f, w=w, first=j, last=j, peak=peak, lo=lo, hi=hi))
    kept = [(e["f"], e["w"], e["first"] * slice_ms, (e["last"] + 1) * slice_ms, e["peak"]) for e in events
            if e["last"] - e["first"] + 1 >= min_slices]
    return sorted(kept, key=lambda e: (e[2], e[0]))


def monitor_pulsed(kurtosis, clip_share, mads=MONITOR_PULSED_MADS):
    """The slices (indices) whose excess kurtosis or clip share stands out of the record's own slices: above the median
    of that figure over the slices + mads x 1.4826 x their median absolute deviation."""
    flagged = np.zeros(len(kurtosis), dtype=bool)
    for v in (np.asarray(kurtosis, dtype=np.float64), np.asarray(clip_share, dtype=np.float64)):
        if v.size:
            med = np.median(v)
            flagged |= v > med + mads * 1.4826 * np.median(np.abs(v - med))
    return [int(j) for j in np.flatnonzero(flagged)]


class FrontEnd(object):
    """The front end of Settings: the two walks over STAGES and the prepared record, then per stage, in the table's order,
    its format check, its design and its public method."""

    def _walk(self, upto=None):
        """The table folded forwards over the file's settings: (steps, settings).  steps: per stage that is on (stage, the
        settings it reads under, n_in, n_out); settings: what the record behind the last of them is read under, with
        skipNumberOfBytes mapped through the pairs - self itself where nothing is on.  upto: the name of a stage to stop in
        front of.  ValueError for what a stage refuses, and for a skipNumberOfBytes that is off a multiple of some n_in."""
        s, steps = self, []
        for stage in STAGES:
            if stage.name == upto:
                break
            if not stage.on(s):
                continue
            n_in, n_out, out = stage.step(s)
            pos = int(s.skipNumberOfBytes)
            if pos % n_in:
                raise ValueError("skipNumberOfBytes = %d splits %s: position %d of the record the %s stage reads must be %s"
                                 % (int(self.skipNumberOfBytes), stage.reads, pos, stage.name, _multiple(n_in)))
            out.skipNumberOfBytes = pos // n_in * n_out
            steps.append((stage, s, n_in, n_out))
            s = out
        return steps, s

    def _prepared_settings(self):
        """The settings the PREPARED record is read under, skipNumberOfBytes turned from a byte of the file into the sample
        of the prepared record it becomes: the end of _walk().  The settings themselves where no stage is on."""
        return self._walk()[1]

    def _file_range(self, offset, count):
        """(first byte, bytes) of the file that samples [offset, offset + count) of the prepared record are made of: the
        pairs of _walk in reverse order, each stage's count rule.  ValueError where `offset` is not a position of every
        record on the way.  Opens nothing."""
        for stage, _, n_in, n_out in reversed(self._walk()[0]):
            if offset % n_out:
                raise ValueError("sample %d of the record the %s stage makes splits %s: it must be %s"
                                 % (offset, stage.name, stage.makes, _multiple(n_out)))
            offset, count = offset // n_out * n_in, stage.count_in(self, count, n_in, n_out)
        return offset, count

    @contextlib.contextmanager
    def _prepared_record(self, name, offset, count, mitigate_at=None, verbose=False):
        """Samples [offset, offset + count) of the prepared record of a record file, uploaded once and prepared on the
        GPU, for the length of the block: the bytes _file_range(offset, count) of the file - offset and count are in BYTES
        OF THE PREPARED RECORD - through every stage of STAGES that is on, each intermediate record freed as soon as the
        next one exists, then with mitigate_at (a sample of the prepared record; None: no mitigation) cleared of the
        narrowband lines in the spectrum from there on - the notch is designed at the prepared rate.  With
        sweptMitigation the record first goes through excise(), so the notch's spectrum is the excised record's; the notch
        then runs only where interferenceMitigation asks for it too.  Yields the prepared record, to be read under
        _prepared_settings(), and frees it afterwards."""
        from . import engine
        say = print if verbose else (lambda *args: None)
        steps, real = self._walk()
        first, n_bytes = self._file_range(offset, count)
        if steps and isinstance(steps[0][0], _Unpack):      # (a packed file that ends inside a frame: the frame is left)
            unit = steps[0][0].whole(self, steps[0][2], steps[0][3])[0]     # (... with antennas, of all antennas)
            n_bytes = min(n_bytes, max(0, os.path.getsize(name) - first) // unit * unit)
        rec = engine.get_context(real, None).upload_file(name, first, n_bytes)
        try:
            for stage, s, _, _ in steps:
                raw, rec = rec, None
                try:
                    rec, info = stage.run(s, raw, say, real)
                finally:
                    raw.free()
                if stage.last:
                    setattr(self, stage.last, info)
            if mitigate_at is not None and self.sweptMitigation:
                say('   Excising swept interference (segments of %d samples)...' % int(self.exciseSegment))
                raw, rec = rec, None
                try:
                    rec, info = real.excise(raw)
                finally:
                    raw.free()
                say('   %.4f %% of the time-frequency cells cut, %d samples clipped'
                    % (100.0 * info["cells_cut"], info["clipped"]))
                self.lastExcision = info
            if mitigate_at is not None and (self.interferenceMitigation or not self.sweptMitigation):
                say('   Looking for narrowband interference...')
                raw = rec
                rec, lines = real.mitigate(raw, offset=min(mitigate_at, len(raw)))
                if rec is not raw:
                    raw.free()
                for f_hz, w_hz in lines:
                    say('   Removed a line at %.4f MHz (notch %.1f kHz wide)' % (f_hz / 1e6, w_hz / 1e3))
                if not lines:
                    say('   No narrowband interference found')
                self.lastNotchLines = lines
                if self.notchWholeRecord:
                    self.lastMonitor = real.lastMonitor
                    for f_hz, w_hz, first_ms, last_ms, peak_db in self.lastMonitor["events"]:
                        say('   Seen from %.0f to %.0f ms: a line at %.4f MHz, %.1f dB over the floor'
                            % (first_ms, last_ms, f_hz / 1e6, peak_db))
            yield rec
        finally:
            if rec is not None:
                rec.free()

    def excise(self, record):
        """Swept (chirp) interference excision of a resident int8 record (a _native.Record; Context.excise_record): segments
        of exciseSegment samples at half that hop under a root-Hann window, in each the bins above exciseThreshold x the
        mean of its kept bins zeroed (excisePasses rounds), overlap-add back.  Returns (record, info): a NEW record of the
        same length - sample n lines up with sample n of the old one - and info, kept as self.lastExcision: segments,
        bins_cut, segments_cut, clipped, cells_cut (the share of the segments x (exciseSegment / 2 - 1) time-frequency
        cells that were cut) and cut_per_segment (uint16 per segment).  The caller frees both records."""
        if np.dtype(self.dataType) != np.dtype(np.int8):
            raise ValueError("swept-interference excision reads int8 records only, not Settings.dataType %r" % (self.dataType,))
        N = int(self.exciseSegment)
        new, info = record.ctx.excise_record(record, N, float(self.exciseThreshold), int(self.excisePasses))
        info["cells_cut"] = info["bins_cut"] / float(info["segments"] * (N // 2 - 1))
        self.lastExcision = info
        return new, info

    def mitigate(self, record, offset=0, device=None):
        """Narrowband interference excision of a resident int8 record (a _native.Record): the Welch spectrum of the 10 code
        periods from sample `offset` (probe_stats, as probeData), its lines by notchThresholdDb / notchWidthHz, a notch of
        notchTaps taps (notch_design) and, if there is a line, the whole record through it (filter_record).  Returns
        (record, lines): a NEW record of the same length - sample n lines up with sample n of the old one - or the SAME
        record when no line was found; lines is a list of (centre Hz, width Hz).  The caller frees what it gets.
        With notchWholeRecord the spectrum is the max-hold over the slices of monitorRecord(record, offset) instead: a line
        that comes up anywhere in the record is notched, not only one present in its first 10 ms."""
        from . import engine
        if np.dtype(self.dataType) != np.dtype(np.int8):
            raise ValueError("interference excision filters int8 records only, not Settings.dataType %r" % (self.dataType,))
        ctx = record.ctx if device is None else engine.get_context(self, device)
        if self.notchWholeRecord:
            seen = self.monitorRecord(record, offset)["waterfall"]
            f, pxx = seen.f, seen.hold
        else:
            n = min(10 * self.samplesPerCode, len(record) - int(offset))
            f, pxx, _, _ = ctx.probe_stats(record, int(offset), n, self.samplingFreq / 1000000.0)
        taps, shift, lines = _native.notch_design(self, f, pxx, self.notchThresholdDb, self.notchWidthHz, self.notchTaps)
        if not lines:
            return record, lines
        return ctx.filter_record(record, taps, shift), lines

    def monitorRecord(self, record, offset=0):
        """The spectrum and the sample statistics of a resident int8 record (a _native.Record) from sample `offset` to its
        end, slice by slice (Context.waterfall): slices of monitorSliceMs, Welch segments of monitorSegment samples that
        share monitorOverlap.  Returns info and keeps it as self.lastMonitor: waterfall (a _native.Waterfall: f, pxx, hold,
        moments, hist, n_segments, mean, rms, kurtosis, clip_share), slice_ms, events and pulsed.
        events: the lines notch_design finds in each slice's spectrum (notchThresholdDb, notchWidthHz), merged across
        consecutive slices where their bands overlap (monitor_events), each (f_hz, width_hz, first_ms, last_ms,
        peak_db_over_floor), ms from `offset`; events shorter than monitorMinSlices slices are dropped.
        pulsed: the slices whose excess kurtosis or share of samples on -128, -127 or +127 lies above the median of that
        figure over the record's own slices + 6 x 1.4826 x its median absolute deviation (monitor_pulsed): the threshold
        comes from the spread of the record, so a steady record of any statistics flags about nothing."""
        if np.dtype(self.dataType) != np.dtype(np.int8):
            raise ValueError("the monitor reads int8 records only, not Settings.dataType %r" % (self.dataType,))
        fs = float(self.samplingFreq)
        S = int(np.rint(float(self.monitorSliceMs) * 1e-3 * fs))
        seen = record.ctx.waterfall(record, int(offset), len(record) - int(offset), fs / 1e6, int(self.monitorSegment),
                                    int(self.monitorOverlap), S)
        per_slice = []
        for pxx in seen.pxx:
            lines = _native.notch_design(self, seen.f, pxx, self.notchThresholdDb, self.notchWidthHz, self.notchTaps)[2]
            per_slice.append([(f_hz, w_hz, line_peak_db(seen.f, pxx, f_hz, w_hz)) for f_hz, w_hz in lines])
        slice_ms = 1e3 * S / fs
        info = dict(waterfall=seen, slice_ms=slice_ms,
                    events=monitor_events(per_slice, slice_ms, int(self.monitorMinSlices)),
                    pulsed=monitor_pulsed(seen.kurtosis, seen.clip_share))
        self.lastMonitor = info
        return info

    def _pack_format(self):
        """(bits, lsb_first, frame, first, take, table) of the unpacker for these settings.  take: a frame of several
        fields (packedFrame > 1) gives its I/Q pair with iqRecord, else one field; with packedFrame = 1 every field is
        taken (I and Q simply alternate, the converter sorts them out).  With Settings.antennas a frame of several fields
        gives that many times as many: the streams of all antennas from `first` on, for the combiner behind the unpacker."""
        b = int(self.packedBits)
        if b not in (1, 2, 4):
            raise ValueError("Settings.packedBits = %r: packed records hold 1-, 2- or 4-bit samples (0: not packed)"
                             % (self.packedBits,))
        if self.iqRequantize:
            raise ValueError("Settings.packedBits with Settings.iqRequantize: the requantiser reads int16 and float32 "
                             "files, a packed file is neither")
        if self.frontEndConditioning:
            raise ValueError("Settings.packedBits with Settings.frontEndConditioning: the front end's own AGC has set the "
                             "levels of a packed file; conditioning it is out of scope")
        if np.dtype(self.dataType) != np.dtype(np.int8):
            raise ValueError("Settings.packedBits makes an int8 record of the file: Settings.dataType stays 'int8', not %r"
                             % (self.dataType,))
        F, first = int(self.packedFrame), int(self.packedFirst)
        if F not in (1, 2, 4, 8, 16):
            raise ValueError("Settings.packedFrame = %r: a frame holds 1, 2, 4, 8 or 16 fields" % (self.packedFrame,))
        take = 2 if (self.iqRecord and F > 1) else 1
        if self.antennas and F > 1:          # (the streams of all antennas, for the combiner behind the unpacker)
            take = self._array_format()[1] * take
        if first < 0 or first + take > F:
            raise ValueError("Settings.packedFirst = %d: %d field%s from there on do not lie inside a frame of %d"
                             % (first, take, "s" if take > 1 else "", F))
        if self.packedTable is not None:
            t = np.asarray(self.packedTable)
            if t.ndim != 1 or t.size != 1 << b or t.dtype.kind not in "iu" or t.min() < -128 or t.max() > 127:
                raise ValueError("Settings.packedTable holds 2^packedBits = %d integers that fit int8" % (1 << b))
            table = t.astype(np.int8)
        else:
            if self.packedEncoding not in _native.UNPACK_ENCODINGS:
                raise ValueError("Settings.packedEncoding = %r is none of %s"
                                 % (self.packedEncoding, ", ".join(sorted(_native.UNPACK_ENCODINGS))))
            peak = int(self.packedPeak)
            if not ((1 << b) - 1 <= peak <= 127):
                raise ValueError("Settings.packedPeak = %r lies outside %d .. 127" % (self.packedPeak, (1 << b) - 1))
            table = _native.unpack_table(b, self.packedEncoding, peak)
        return b, bool(self.packedLsbFirst), F, first, take, table

    def _pack_units(self):
        """(bytes of the file, samples of the unpacked record they become): the smallest run of whole bytes that holds
        whole frames, max(1, F b / 8) bytes."""
        b, _, F, _, take, _ = self._pack_format()
        unit = max(1, F * b // 8)
        return unit, unit * 8 * take // (b * F)

    def unpackRecord(self, record):
        """A resident record holding the raw bytes of a packed file (a _native.Record; packedBits, packedLsbFirst,
        packedFrame, packedFirst say how, packedEncoding and packedPeak, or packedTable, what a code means) as a NEW int8
        record, one sample per selected field (Context.unpack).  Returns (record8, info) and keeps info as
        self.lastUnpack: samples, bits, table (int8 per code), code_counts (int64 per code, exact) and shares (each code's
        share of the samples - the histogram of the ADC's levels: of a 2-bit front end whose AGC works about one third
        lies in the outer levels).  The caller frees both."""
        if not self.packedBits:
            raise ValueError("Settings.packedBits is 0: the record is not packed")
        b, lsb, F, first, take, table = self._pack_format()
        rec8 = record.ctx.unpack(record, b, table, lsb_first=lsb, frame=F, first=first, take=take)
        counts = rec8.code_counts
        info = dict(samples=len(rec8), bits=b, table=table.copy(), code_counts=counts.copy(),
                    shares=counts / float(len(rec8)) if len(rec8) else np.zeros(counts.size))
        self.lastUnpack = info
        return rec8, info

    def _array_format(self):
        """(lanes, A, K, reference, offset_binary) of the antenna combiner for these settings."""
        if self.frontEndConditioning or self.iqRequantize:
            raise ValueError("Settings.antennas with Settings.%s: a gain of its own per stream would destroy the coherence "
                             "of the streams that the combiner's null rests on"
                             % ("frontEndConditioning" if self.frontEndConditioning else "iqRequantize"))
        try:
            A, K, ref = int(self.antennas), int(self.arrayTaps), int(self.arrayReference)
            ok = A == self.antennas and 2 <= A <= _native.ARRAY_MAX_ANTENNAS
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("Settings.antennas = %r: the number of antennas is an integer in 2 .. %d (0: the stage is off)"
                             % (self.antennas, _native.ARRAY_MAX_ANTENNAS))
        dt = np.dtype(self.dataType)
        if dt not in (np.dtype(np.int8), np.dtype(np.uint8)):
            raise ValueError("a multi-antenna record (Settings.antennas) holds int8 samples, or uint8 for offset binary, not "
                             "Settings.dataType %r: int16 and float multi-antenna files are out of scope" % (self.dataType,))
        if K == 0:
            K = 1 if self.iqRecord else 5
        if K != (self.arrayTaps or K) or not (1 <= K <= _native.ARRAY_MAX_TAPS and K % 2 == 1):
            raise ValueError("Settings.arrayTaps = %r: the taps per antenna are odd, 1 .. %d (0: 1 for an I/Q record, else 5)"
                             % (self.arrayTaps, _native.ARRAY_MAX_TAPS))
        if A * K > _native.ARRAY_MAX_WEIGHTS:
            raise ValueError("Settings.antennas x Settings.arrayTaps = %d x %d: more than %d weights"
                             % (A, K, _native.ARRAY_MAX_WEIGHTS))
        if ref != self.arrayReference or not (0 <= ref < A):
            raise ValueError("Settings.arrayReference = %r is none of the antennas 0 .. %d" % (self.arrayReference, A - 1))
        loading, target = float(self.arrayLoading), float(self.arrayTargetRms)
        if not (np.isfinite(loading) and loading >= 0):
            raise ValueError("Settings.arrayLoading = %r: the diagonal loading is finite and not negative" % (self.arrayLoading,))
        if not (0 < target <= 127.0):
            raise ValueError("Settings.arrayTargetRms = %r lies outside (0, 127]" % (self.arrayTargetRms,))
        self._array_block_format()
        return 2 if self.iqRecord else 1, A, K, ref, dt == np.dtype(np.uint8)

    def _array_block_format(self):
        """(block length in frames, window in blocks) of the block-adaptive combiner for these settings, or None where
        arrayBlockMs is 0: one set of weights per record."""
        try:
            ms = float(self.arrayBlockMs)
            ok = np.isfinite(ms) and ms >= 0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("Settings.arrayBlockMs = %r: the block length in ms is finite and not negative (0: one set of "
                             "weights per record)" % (self.arrayBlockMs,))
        try:
            W = int(self.arrayWindowBlocks)
            ok = W == self.arrayWindowBlocks and 1 <= W <= _native.ARRAY_MAX_WINDOW and W % 2 == 1
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("Settings.arrayWindowBlocks = %r: the window is an odd number of blocks in 1 .. %d"
                             % (self.arrayWindowBlocks, _native.ARRAY_MAX_WINDOW))
        if ms == 0:
            return None
        unit = _native.ARRAY_BLOCK_UNIT                # (the rate of frames is samplingFreq for a real and an I/Q record alike)
        return max(1, int(round(ms * float(self.samplingFreq) / 1000.0 / unit))) * unit, W

    def combineAntennas(self, record):
        """A resident int8 record that interleaves the streams of Settings.antennas antennas frame by frame (a
        _native.Record; with iqRecord every stream is interleaved I/Q, uint8 is read as offset binary) as a NEW int8
        record of one stream: the exact lag statistics of the streams (Context.array_stats), the power-inversion weights
        of arrayTaps taps per antenna with antenna arrayReference held at 1 (_native.array_design; arrayLoading,
        arrayTargetRms), every stream through its taps and all of them summed (Context.combine).  Output frame f is the
        instant of input frame f.  Returns (record8, info) and keeps info as self.lastCombining: samples, antennas, taps
        (per antenna), reference, weights (antennas x taps, complex for I/Q, before the gain), gain_db, suppression_db (the
        reference antenna's power over the output's), input_rms (per antenna and component, LSB) and clipped (share of the
        samples that left the int8 range).  With arrayBlockMs the weights change along the record, block by block
        (_combine_blocks says what the info holds then).  The caller frees both."""
        if not self.antennas:
            raise ValueError("Settings.antennas is 0: the stage is off")
        lanes, A, K, ref, offset_binary = self._array_format()
        if len(record) % (A * lanes):
            raise ValueError("a record of %d antennas holds whole frames of %d bytes, not %d bytes" % (A, A * lanes, len(record)))
        ctx = record.ctx
        frames = len(record) // (A * lanes)
        blocks = self._array_block_format()
        if blocks is not None:
            return self._combine_blocks(record, frames, *blocks)
        rho = ctx.array_stats(record, lanes, A, K, offset_binary=offset_binary)
        try:
            taps, shift, out = _native.array_design(rho, frames, lanes, ref, self.arrayLoading, self.arrayTargetRms)
        except _native.SgxError as e:
            raise ValueError("Settings.antennas = %d, arrayTaps = %d, arrayReference = %d, arrayLoading = %r, arrayTargetRms = %r "
                             "on a record of %d frames: %s" % (A, K, ref, self.arrayLoading, self.arrayTargetRms, frames, e))
        rec8 = ctx.combine(record, lanes, A, taps, shift, offset_binary=offset_binary)
        power = np.array([float(rho[a, a, 0, 0]) for a in range(A)])
        info = dict(samples=len(rec8), antennas=A, taps=K, reference=ref, weights=out["weights"],
                    gain_db=20.0 * float(np.log10(out["gain"])), suppression_db=out["suppression_db"],
                    input_rms=np.sqrt(power / (float(frames) * lanes)),
                    clipped=float(rec8.clipped) / len(rec8) if len(rec8) else 0.0)
        self.lastCombining = info
        return rec8, info

    def _combine_blocks(self, record, frames, B, W):
        """combineAntennas with arrayBlockMs: the statistics of every block of B frames (Context.array_block_stats), a set
        of weights per block from the statistics of the W blocks around it (_native.array_design_blocks) and every output
        frame through the set of its block (Context.combine_blocks).  Blocks count from the first frame of `record`.
        lastCombining keeps its keys, with weights (blocks x antennas x taps) and suppression_db and gain_db the medians
        over the designed blocks, and gains block_frames, blocks, window_blocks, block_suppression_db, block_gain_db,
        held_blocks (blocks that hold a neighbour's weights: their own window is all zero) and suppression_db_min."""
        lanes, A, K, ref, offset_binary = self._array_format()
        ctx = record.ctx
        rho = ctx.array_block_stats(record, lanes, A, K, B, offset_binary=offset_binary)
        try:
            taps, shift, out = _native.array_design_blocks(rho, frames, B, W, lanes, ref, self.arrayLoading, self.arrayTargetRms)
        except _native.SgxError as e:
            raise ValueError("Settings.antennas = %d, arrayTaps = %d, arrayReference = %d, arrayLoading = %r, arrayTargetRms = %r, "
                             "arrayBlockMs = %r (%d frames), arrayWindowBlocks = %d on a record of %d frames: %s"
                             % (A, K, ref, self.arrayLoading, self.arrayTargetRms, self.arrayBlockMs, B, W, frames, e))
        rec8 = ctx.combine_blocks(record, lanes, A, taps, B, shift, offset_binary=offset_binary)
        power = np.array([float(rho[:, a, a, 0, 0].sum()) for a in range(A)])
        designed = out["status"] == 0
        gain_db = 20.0 * np.log10(out["gain"])
        info = dict(samples=len(rec8), antennas=A, taps=K, reference=ref, weights=out["weights"],
                    gain_db=float(np.median(gain_db[designed])), suppression_db=float(np.median(out["suppression_db"][designed])),
                    suppression_db_min=float(np.min(out["suppression_db"][designed])),
                    input_rms=np.sqrt(power / (float(frames) * lanes)),
                    clipped=float(rec8.clipped) / len(rec8) if len(rec8) else 0.0,
                    block_frames=B, blocks=int(rho.shape[0]), window_blocks=W, block_suppression_db=out["suppression_db"],
                    block_gain_db=gain_db, held_blocks=int(np.count_nonzero(out["status"])))
        self.lastCombining = info
        return rec8, info

    def _cond_format(self):
        """(bytes per component, lanes, block in frames, blank_q4) of the conditioning stage for these settings."""
        dt = np.dtype(self.dataType)
        if self.iqRequantize:
            raise ValueError("Settings.frontEndConditioning stands where the fixed-gain requantiser (Settings.iqRequantize) "
                             "does: not both")
        if dt == np.dtype(np.float32):
            raise ValueError("Settings.frontEndConditioning reads int8, uint8 and int16 records: float32 sums are not "
                             "order-free, so Settings.dataType 'float32' goes through Settings.iqRequantize instead")
        w = _native.cond_type(dt)[1]
        block = 16 * int(np.rint(float(self.condBlockUs) * 1e-6 * float(self.samplingFreq) / 16.0))
        c = float(self.condBlankFactor)
        return w, 2 if self.iqRecord else 1, min(16384, max(256, block)), int(np.rint(16.0 * c * c))

    def conditionRecord(self, record):
        """A resident record holding the raw bytes of an int8, uint8 or int16 file (a _native.Record; Settings.dataType
        says which; with iqRecord interleaved I/Q) as a NEW int8 record, one sample per component, conditioned block by
        block: the statistics of every block of condBlockUs (cond_stats), smoothed over condAgcBlocks blocks into a DC per
        rail, a gain that brings the rms to condTargetRms and a blanking threshold of condBlankFactor x the rms
        (cond_plan), and the record through them, frames within condGuardFrames of a hit set to zero (condition).  Sample
        n of the new record is component n of the file.  Returns (record8, info) and keeps info as self.lastConditioning:
        samples, block, blocks, blank_q4, blanked (share of the frames), clipped (share of the samples on +-127), gain_db_min,
        gain_db_max, dc_min and dc_max (a tuple per lane, LSB).  The caller frees both."""
        if not self.frontEndConditioning:
            raise ValueError("Settings.frontEndConditioning is off")
        w, lanes, block, blank_q4 = self._cond_format()
        dt = np.dtype(self.dataType)
        ctx = record.ctx
        stats = ctx.cond_stats(record, dt, lanes, block, blank_q4)
        plan = _native.cond_plan(stats, lanes, blank_q4, self.condTargetRms, self.condAgcBlocks)
        rec8 = ctx.condition(record, dt, lanes, block, plan, int(self.condGuardFrames))
        frames = len(rec8) // lanes
        info = dict(samples=len(rec8), block=block, blocks=int(plan.size), blank_q4=blank_q4,
                    blanked=float(rec8.blanked) / frames if frames else 0.0,
                    clipped=float(rec8.clipped) / len(rec8) if len(rec8) else 0.0)
        if plan.size:
            gain_db = 20.0 * np.log10(plan["mult"].astype(np.float64) / np.exp2(plan["shift"].astype(np.float64)))
            info["gain_db_min"], info["gain_db_max"] = float(gain_db.min()), float(gain_db.max())
            dcs = [plan[k].astype(np.float64) / 16.0 for k in ("dc0", "dc1")[:lanes]]
            info["dc_min"], info["dc_max"] = tuple(float(d.min()) for d in dcs), tuple(float(d.max()) for d in dcs)
        else:
            info["gain_db_min"] = info["gain_db_max"] = 0.0
            info["dc_min"] = info["dc_max"] = (0.0,) * lanes
        self.lastConditioning = info
        return rec8, info

    def _iq_width(self):
        """Bytes per component of the I/Q file: 2 or 4 where it goes through the requantiser or the conditioning stage,
        else 1."""
        self._iq_format()
        return np.dtype(self.dataType).itemsize if self.iqRecord else 1

    def requantizeIQ(self, record):
        """A resident record holding the raw bytes of an int16 or float32 file (a _native.Record; Settings.dataType says
        which) as a NEW int8 record, one sample per component: the statistics of the whole record (requant_stats), the
        fixed gain that brings its rms to iqTargetRms (requant_gain), the record through it (requantize).  Sample n of the
        new record is component n of the file, i.e. file byte n w for w-byte components.  Returns (record8, info) and keeps
        info as self.lastRequant: the statistics (n_finite, n_nonfinite, max_abs, sum, sum_sq), rms, mult and shift (int16)
        or scale (float32), gain_db, and clipped, the share of the samples that landed on +-127.  The caller frees both."""
        if not self.iqRequantize:
            raise ValueError("Settings.iqRequantize is off: int16 and float32 I/Q are not converted to int8")
        dt = np.dtype(self.dataType)
        ctx = record.ctx
        info = ctx.requant_stats(record, dt)
        mult, shift, scale = _native.requant_gain(info, dt, self.iqTargetRms)
        rec8 = ctx.requantize(record, dt, mult=mult, shift=shift, scale=scale)
        info["rms"] = float(np.sqrt(info["sum_sq"] / info["n_finite"])) if info["n_finite"] else 0.0
        if dt == np.dtype(np.int16):
            info["mult"], info["shift"] = mult, shift
            gain = float(mult) / float(1 << shift)
        else:
            info["scale"] = scale
            gain = float(scale)
        info["gain_db"] = 20.0 * float(np.log10(gain))
        info["clipped"] = float(rec8.clipped) / len(rec8) if len(rec8) else 0.0
        self.lastRequant = info
        return rec8, info

    def _decim_format(self):
        """(lanes, D, taps, offset_binary, q_first) of the decimation stage for these settings: what the record is where
        the stage sees it, behind the unpacker, the conditioning stage and the requantiser."""
        try:
            D = int(self.decimation)
            ok = D == self.decimation and _native.DECIM_MIN_FACTOR <= D <= _native.DECIM_MAX_FACTOR
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("Settings.decimation = %r: the factor is an integer in %d .. %d (0: the stage is off)"
                             % (self.decimation, _native.DECIM_MIN_FACTOR, _native.DECIM_MAX_FACTOR))
        L = int(self.decimTaps)
        if L != self.decimTaps or not (1 <= L <= _native.DECIM_MAX_TAPS and L % 2 == 1):
            raise ValueError("Settings.decimTaps = %r: the filter length is odd, 1 .. %d" % (self.decimTaps,
                                                                                           _native.DECIM_MAX_TAPS))
        if self.iqRecord:
            q_first, offset_binary = self._iq_format()       # (raises for what does not reach the converter either)
            return 2, D, L, offset_binary, q_first
        if self.frontEndConditioning:
            self._cond_format()                              # (what conditionRecord makes of the file is int8)
        elif np.dtype(self.dataType) != np.dtype(np.int8):
            raise ValueError("Settings.decimation reads a real record as int8: Settings.dataType %r is decimated only behind "
                             "Settings.frontEndConditioning (int8, uint8, int16) or as a packed file (Settings.packedBits)"
                             % (self.dataType,))
        return 1, D, L, False, False

    def _decim_design(self):
        """(taps, shift, info) of the decimation filter for these settings: the band decimBandwidth wide around IF
        (_native.decim_design; info: fs_out, f_out, inverted).  For a Q-first I/Q file the taps are conjugated: filtering
        Q + jI with conj(h) gives Im w + j Re w, a Q-first record again."""
        lanes, D, L, _, q_first = self._decim_format()
        try:
            taps, shift, info = _native.decim_design(self.samplingFreq, self.IF, self.decimBandwidth, lanes, D, L,
                                                     self.decimGain)
        except _native.SgxError as e:
            raise ValueError("Settings.decimation = %d, decimTaps = %d, decimBandwidth = %r, decimGain = %r at samplingFreq "
                             "%r, IF %r: %s" % (D, L, self.decimBandwidth, self.decimGain, self.samplingFreq, self.IF, e))
        if q_first:
            taps[1::2] = -taps[1::2]
        return taps, shift, info

    def decimateRecord(self, record):
        """A resident int8 record (a _native.Record; with iqRecord interleaved I/Q, uint8 read as offset binary) as a NEW
        int8 record at 1 / decimation of the rate: the band decimBandwidth wide around IF through a decimTaps-tap band-pass
        (decim_design), every decimation-th output kept (Context.decimate).  Output frame m is the instant of input frame
        m decimation.  Returns (record8, info) and keeps info as self.lastDecimation: factor, taps (the filter length),
        fs_out, f_out (rate and IF - for I/Q the offset - of the new record), inverted (the band came out mirrored: the
        Doppler it shows has the other sign), clipped (share of the samples that left the int8 range) and samples.  The
        caller frees both."""
        if not self.decimation:
            raise ValueError("Settings.decimation is 0: the stage is off")
        lanes, D, L, offset_binary, _ = self._decim_format()
        taps, shift, out = self._decim_design()
        rec8 = record.ctx.decimate(record, lanes, taps, shift, D, offset_binary=offset_binary)
        info = dict(factor=D, taps=L, fs_out=out["fs_out"], f_out=out["f_out"], inverted=out["inverted"],
                    clipped=float(rec8.clipped) / len(rec8) if len(rec8) else 0.0, samples=len(rec8))
        self.lastDecimation = info
        return rec8, info

    def _iq_format(self):
        """(q_first, offset_binary) of the I/Q file these settings describe."""
        dt = np.dtype(self.dataType)
        if self.frontEndConditioning:
            self._cond_format()
            return bool(self.iqQFirst), False        # (what conditionRecord makes of the file is int8, its offset removed)
        if self.iqRequantize and dt in (np.dtype(np.int16), np.dtype(np.float32)):
            return bool(self.iqQFirst), False        # (what requantizeIQ makes of the file is int8)
        if dt not in (np.dtype(np.int8), np.dtype(np.uint8)):
            if self.iqRequantize:
                raise ValueError("an I/Q record (Settings.iqRecord) holds int8 samples, uint8 for offset binary or, with "
                                 "Settings.iqRequantize, int16 or float32, not Settings.dataType %r" % (self.dataType,))
            raise ValueError("an I/Q record (Settings.iqRecord) holds int8 samples, or uint8 for offset binary, not "
                             "Settings.dataType %r: int16 and float32 I/Q are not converted" % (self.dataType,))
        return bool(self.iqQFirst), dt == np.dtype(np.uint8)

    def realEquivalent(self):
        """The settings of the real IF record that convertIQ makes of the I/Q file these settings describe: a copy with
        samplingFreq * 2, IF + samplingFreq / 2, iqRecord = False and dataType 'int8' (what the converter writes).
        Without iqRecord the record is real already: a plain copy."""
        if not self.iqRecord:
            return copy.copy(self)
        return _with(self, samplingFreq=2.0 * self.samplingFreq, IF=self.IF + self.samplingFreq / 2.0, iqRecord=False,
                     dataType='int8')

    def convertIQ(self, record):
        """A resident record holding the raw bytes of an interleaved 8-bit I/Q file (a _native.Record) as the equivalent
        real IF record (iq_to_if through the iqTaps-tap filter of iq_design): a NEW int8 record of the same length whose
        sample n is the instant of byte n's pair, to be read under realEquivalent().  The caller frees both."""
        q_first, offset_binary = self._iq_format()
        taps, shift = _native.iq_design(self.iqTaps)
        return record.ctx.iq_to_if(record, taps, shift, q_first=q_first, offset_binary=offset_binary)

    def _resamp_format(self):
        """(L, M, taps) of the resampling stage for these settings: the pair resampleUp / resampleDown and the filter
        length, resampTaps or 24 L + 1."""
        try:
            L, M = int(self.resampleUp), int(self.resampleDown)
            ok = L == self.resampleUp and M == self.resampleDown and _native.resamp_pair_ok(L, M)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("Settings.resampleUp / Settings.resampleDown = %r / %r: the ratio L / M has 1 <= M <= %d, "
                             "M < L <= %d and no common factor (resampleUp = 0: the stage is off)"
                             % (self.resampleUp, self.resampleDown, _native.RESAMP_MAX_DOWN, _native.RESAMP_MAX_UP))
        try:
            Lh = int(self.resampTaps)
            ok = Lh == self.resampTaps and (Lh == 0 or (1 <= Lh <= _native.RESAMP_MAX_TAPS and Lh % 2 == 1))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("Settings.resampTaps = %r: the filter length is odd, 1 .. %d (0: 24 resampleUp + 1)"
                             % (self.resampTaps, _native.RESAMP_MAX_TAPS))
        return L, M, Lh if Lh else 24 * L + 1

    def _resamp_design(self):
        """(taps, shift, info) of the resampling filter for these settings (_native.resamp_design at the rate of the
        record the stage reads, a real int8 record; info: fs_out, cutoff).  The C/A band of that record, up to
        IF + 1.023 MHz, must lie below the cutoff."""
        L, M, Lh = self._resamp_format()
        front = self._walk(upto=_Resample.name)[1]
        if np.dtype(front.dataType) != np.dtype(np.int8):
            raise ValueError("Settings.resampleUp reads a real record as int8: Settings.dataType %r is resampled only behind a "
                             "stage that makes int8 of it (Settings.frontEndConditioning, Settings.packedBits, "
                             "Settings.iqRecord)" % (front.dataType,))
        fs = float(front.samplingFreq)
        try:
            taps, shift, info = _native.resamp_design(fs, L, M, Lh, self.resampCutoff, self.resampGain)
        except (_native.SgxError, TypeError, ValueError) as e:
            raise ValueError("Settings.resampleUp / resampleDown = %d / %d, resampTaps = %d, resampCutoff = %r, resampGain = %r "
                             "at samplingFreq %r: %s" % (L, M, Lh, self.resampCutoff, self.resampGain, fs, e))
        cutoff = float(self.resampCutoff) if self.resampCutoff else min(fs, info["fs_out"]) / 2.0
        if not float(front.IF) + 1.023e6 < cutoff:
            raise ValueError("Settings.resampCutoff: the low-pass of the resampler cuts off at %.6g Hz, at or below the upper "
                             "edge of the C/A band, IF + 1.023 MHz = %.6g Hz" % (cutoff, float(front.IF) + 1.023e6))
        info["cutoff"] = cutoff
        return taps, shift, info

    def resampleRecord(self, record):
        """A resident real int8 record (a _native.Record) as a NEW int8 record at resampleUp / resampleDown of the rate,
        through the resampTaps-tap low-pass of resamp_design (Context.resample).  Output sample m is the instant of input
        position m resampleDown / resampleUp.  Returns (record8, info) and keeps info as self.lastResampling: up, down,
        taps (the filter length), fs_out, clipped (share of the samples that left the int8 range) and samples.  The
        caller frees both."""
        if not self.resampleUp:
            raise ValueError("Settings.resampleUp is 0: the stage is off")
        L, M, Lh = self._resamp_format()
        taps, shift, out = self._resamp_design()
        rec8 = record.ctx.resample(record, taps, shift, L, M)
        info = dict(up=L, down=M, taps=Lh, fs_out=out["fs_out"],
                    clipped=float(rec8.clipped) / len(rec8) if len(rec8) else 0.0, samples=len(rec8))
        self.lastResampling = info
        return rec8, info
