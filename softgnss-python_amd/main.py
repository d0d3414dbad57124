"""The reference's main.py (banner, probeData, postProcessing) for this engine:

    python -m softgnss-python_amd.main record.bin [--fs 38192000 --IF 9548000 --ms 37000 --channels 8 --skip 0]
                                                  [--lock-detector] [--acq-coherent-ms T --acq-blocks M --acq-noncoh]
                                                  [--correlator-bank LO:HI:STEP] [--notch[=THRESHOLD_DB]]
                                                  [--iq[=qi]] [--dtype int8] [--iq-requantize[=RMS]]
                                                  [--condition[=BLANK_FACTOR]]
                                                  [--packed BITS --packed-encoding ENC --packed-lsb-first
                                                   --packed-frame F[:FIRST] --packed-peak PEAK]
                                                  [--decimate D[:TAPS] --decimate-bandwidth HZ]
                                                  [--resample L[/M][:TAPS] --resample-cutoff HZ]

Prints the channel table, the tracking time (with --lock-detector: each channel's C/N0, carrier lock and the time it
was lost, lost channels leaving the navigation) and, when the record is long enough (36 s, four satellites with
ephemerides), the mean position fix.  --correlator-bank=-1:1:0.25 replays the tracked channels at those code offsets
(chips) and prints each channel's mean correlation envelope per tap, normalised to its maximum.  --notch looks for
continuous-wave lines in the record's spectrum (8 dB above the local median, or --notch=THRESHOLD_DB), filters them out on
the GPU before acquisition and tracking, and prints the lines it removed.  --iq reads the file as interleaved 8-bit I/Q
(--iq=qi: Q before I; --dtype uint8: offset binary, as an RTL-SDR writes it): --fs is then the COMPLEX rate and --IF the
baseband offset of the carrier (0 for a zero-IF front end); the GPU turns the file into the equivalent real record at
twice the rate, whose rate and IF are printed, and everything else runs on that.  --iq-requantize (with --iq and --dtype
int16 or float32: sc16 and fc32 captures) first brings the file to int8 on the GPU through one fixed gain that puts its rms
at 12 LSB (or --iq-requantize=RMS), and prints the record's rms, peak, count of non-finite samples, the gain in dB and the
share of clipped samples; --skip stays a byte of the file (a multiple of 4 for int16, 8 for float32), the positions in the
results are samples of the converted record, file byte / 2 or / 4.  --condition (--dtype int8, uint8 or int16, real or
with --iq) first conditions the file block by block on the GPU: per 100 us it removes the DC of each rail, sets the gain
that puts the rms at 12 LSB (a time-varying AGC) and zeroes the frames that stand 4 x (or --condition=BLANK_FACTOR, 1 .. 16;
0: no blanking) above the rms, and prints the span of the gain and the shares of blanked frames and clipped samples; it
stands where --iq-requantize does, so not both; an int16 file is then read as int8, positions are file byte / 2.
--packed BITS (1, 2 or 4; real or with --iq) reads a file of packed samples: the GPU unpacks it first of all into one int8
sample per field, through the levels of --packed-encoding (sign-magnitude, offset-binary or twos-complement) scaled to
--packed-peak (48), the first sample of a byte in its high bits (--packed-lsb-first: in its low bits), and prints the share
of the samples on each level.  --packed-frame F[:FIRST] is for files that interleave several streams: of every F fields (2,
4, 8 or 16) the one at FIRST is kept (with --iq the pair from FIRST on).  --skip stays a byte of the file, on a frame
boundary; positions in the results are samples of the unpacked record.  Not with --iq-requantize or --condition.
--decimate D[:TAPS] (D = 2 .. 16; real int8 records, or with --iq, --condition, --packed) selects the band
--decimate-bandwidth wide (2.046 MHz) around the carrier with a TAPS-tap band-pass (127) on the GPU and keeps every D-th
sample, behind the other preparing stages and in front of the I/Q converter and the notch: everything else runs at 1 / D of
the rate.  The new rate, where the carrier lands, whether the band came out inverted (the Doppler then shows with the other
sign) and the share of clipped samples are printed.  --skip stays a byte of the file, on a multiple of D frames; positions in
the results are samples of the prepared record, D input frames each.  A --fs / --IF pair whose band would alias onto itself at
this D is refused (the default record at D = 2 or 4: use 3 or 5).
--resample L[/M][:TAPS] (L = 2 .. 16, M = 1 .. 3 below L and coprime to it) brings the real int8 record - the file, or what
the stages above make of it - to L / M of its rate on the GPU through a TAPS-tap low-pass (24 L + 1) that cuts off at
--resample-cutoff (half the lower of the two rates), in front of the notch: a capture below the 15.4 samples per chip the
fast tracking kernels need reaches them (4.096 Msps: 10, 16.368 Msps: 7/3, 2.048 Msps I/Q: --iq with 10).  The new rate and
the share of clipped samples are printed.  --skip stays a byte of the file, on a sample that maps to a whole one (a
multiple of M); positions in the results are samples of the resampled record."""
from __future__ import print_function

import argparse

import numpy as np

from . import initialize


def probe_iq(settings):
    """probeData() of an I/Q, a packed or a decimated file: the first 10 code periods prepared on the GPU, probed as the real int8
    record they become."""
    from .record import DeviceSignal
    real = settings._prepared_settings()
    with settings._prepared_record(settings.fileName, int(real.skipNumberOfBytes), 10 * real.samplesPerCode) as rec:
        return real.probeData(DeviceSignal(rec))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("fileName")
    ap.add_argument("--fs", type=float, default=None, help="samplingFreq [Hz]")
    ap.add_argument("--IF", type=float, default=None, help="intermediate frequency [Hz]")
    ap.add_argument("--ms", type=float, default=None, help="msToProcess")
    ap.add_argument("--channels", type=int, default=None, help="numberOfChannels")
    ap.add_argument("--skip", type=int, default=None, help="skipNumberOfBytes")
    ap.add_argument("--no-probe", action="store_true", help="skip the raw-data statistics")
    ap.add_argument("--lock-detector", action="store_true",
                    help="estimate C/N0 per channel, print it after tracking and drop the channels lost on the way")
    ap.add_argument("--acq-coherent-ms", type=int, default=None,
                    help="acquisition: ms summed coherently per window (weak signals: 10; Doppler step 500 / T Hz)")
    ap.add_argument("--acq-blocks", type=int, default=None, help="acquisition: number of windows (reference: 2)")
    ap.add_argument("--acq-noncoh", action="store_true", help="acquisition: sum the windows non-coherently")
    ap.add_argument("--correlator-bank", default=None, metavar="LO:HI:STEP",
                    help="after tracking, replay every channel at code offsets LO .. HI (chips, at most 64 taps) and "
                         "print the mean envelope per tap (a negative LO needs the = form: --correlator-bank=-1:1:0.25)")
    ap.add_argument("--notch", nargs="?", type=float, const=-1.0, default=None, metavar="THRESHOLD_DB",
                    help="excise narrowband interference before acquisition: notch out the spectral lines that stand "
                         "THRESHOLD_DB (default: Settings.notchThresholdDb, 8) above the local median")
    ap.add_argument("--iq", nargs="?", const="iq", default=None, choices=("iq", "qi"), metavar="qi",
                    help="the file is interleaved 8-bit I/Q (--iq=qi: Q first): --fs is the complex rate, --IF the "
                         "baseband offset; it is converted to real IF at twice the rate on the GPU")
    ap.add_argument("--dtype", default=None,
                    help="dataType of the file's samples (numpy name; with --iq: int8 or uint8, with --iq-requantize also "
                         "int16 or float32)")
    ap.add_argument("--iq-requantize", nargs="?", type=float, const=-1.0, default=None, metavar="RMS",
                    help="with --iq and --dtype int16 or float32: bring the file to int8 on the GPU through one fixed gain "
                         "that puts its rms at RMS LSB (default: Settings.iqTargetRms, 12)")
    ap.add_argument("--condition", nargs="?", type=float, const=-1.0, default=None, metavar="BLANK_FACTOR",
                    help="condition the file block by block on the GPU before anything else: DC removal, AGC and pulse "
                         "blanking at BLANK_FACTOR x the rms (default: Settings.condBlankFactor, 4; 0: no blanking)")
    ap.add_argument("--packed", type=int, default=None, choices=(1, 2, 4), metavar="BITS",
                    help="the file holds packed BITS-bit samples (1, 2 or 4): unpack it to int8 on the GPU before anything "
                         "else")
    ap.add_argument("--packed-encoding", default=None, choices=("sign-magnitude", "offset-binary", "twos-complement"),
                    help="with --packed: what a code means (default: Settings.packedEncoding, sign-magnitude)")
    ap.add_argument("--packed-lsb-first", action="store_true",
                    help="with --packed: the first sample of a byte lies in its low bits")
    ap.add_argument("--packed-frame", default=None, metavar="F[:FIRST]",
                    help="with --packed: the file interleaves streams in frames of F fields (1, 2, 4, 8 or 16); keep the "
                         "field at FIRST (default 0; with --iq the I/Q pair from there on)")
    ap.add_argument("--packed-peak", type=int, default=None, metavar="PEAK",
                    help="with --packed: the largest level of the int8 record (default: Settings.packedPeak, 48)")
    ap.add_argument("--decimate", default=None, metavar="D[:TAPS]",
                    help="select the band around the carrier and decimate the record by D (2 .. 16) on the GPU, through a "
                         "band-pass of TAPS taps (odd, at most 511; default: Settings.decimTaps, 127)")
    ap.add_argument("--decimate-bandwidth", type=float, default=None, metavar="HZ",
                    help="with --decimate: the two-sided bandwidth that is kept (default: Settings.decimBandwidth, 2.046e6)")
    ap.add_argument("--resample", default=None, metavar="L[/M][:TAPS]",
                    help="bring the real int8 record to L / M of its rate on the GPU (L 2 .. 16, M 1 .. 3, M < L, coprime), "
                         "through a low-pass of TAPS taps (odd, at most 1023; default: 24 L + 1)")
    ap.add_argument("--resample-cutoff", type=float, default=None, metavar="HZ",
                    help="with --resample: the cutoff of the low-pass (default: half the lower of the two rates)")
    a = ap.parse_args(argv)
    frame = first = None
    up = down = resamp_taps = None
    if a.resample is None:
        if a.resample_cutoff is not None:
            ap.error("--resample-cutoff describes the low-pass of --resample: it needs --resample")
    else:
        try:
            ratio, _, tail = a.resample.partition(":")
            num, _, den = ratio.partition("/")
            up, down = int(num), (int(den) if "/" in ratio else 1)
            resamp_taps = int(tail) if ":" in a.resample else None
            ok = initialize._native.resamp_pair_ok(up, down) and \
                (resamp_taps is None or (1 <= resamp_taps <= 1023 and resamp_taps % 2 == 1))
        except ValueError:
            ok = False
        if not ok:
            ap.error("--resample takes L[/M][:TAPS] with L in 2 .. 16, M in 1 .. 3 below L and coprime to it, and TAPS odd, "
                     "1 .. 1023")
        if a.resample_cutoff is not None and not (np.isfinite(a.resample_cutoff) and a.resample_cutoff > 0):
            ap.error("--resample-cutoff takes the cutoff in Hz, above 0")
        if a.correlator_bank is not None:
            ap.error("--correlator-bank replays from the record file, which --resample resamples on the way in: not both")
    decim = decim_taps = None
    if a.decimate is None:
        if a.decimate_bandwidth is not None:
            ap.error("--decimate-bandwidth describes the band --decimate keeps: it needs --decimate")
    else:
        try:
            parts = [int(x) for x in a.decimate.split(":")]
            decim, decim_taps = parts[0], (parts[1] if len(parts) > 1 else None)
            ok = len(parts) <= 2 and 2 <= decim <= 16 and (decim_taps is None or (1 <= decim_taps <= 511 and decim_taps % 2 == 1))
        except ValueError:
            ok = False
        if not ok:
            ap.error("--decimate takes D[:TAPS] with D in 2 .. 16 and TAPS odd, 1 .. 511")
        if a.decimate_bandwidth is not None and not (np.isfinite(a.decimate_bandwidth) and a.decimate_bandwidth > 0):
            ap.error("--decimate-bandwidth takes the two-sided bandwidth in Hz, above 0")
        if a.correlator_bank is not None:
            ap.error("--correlator-bank replays from the record file, which --decimate resamples on the way in: not both")
    if a.packed is None:
        if a.packed_encoding is not None or a.packed_lsb_first or a.packed_frame is not None or a.packed_peak is not None:
            ap.error("--packed-encoding, --packed-lsb-first, --packed-frame and --packed-peak describe a packed file: "
                     "they need --packed")
    else:
        if a.iq_requantize is not None or a.condition is not None:
            ap.error("--packed makes the int8 record itself: not with --iq-requantize or --condition")
        if a.dtype not in (None, "int8"):
            ap.error("--packed makes an int8 record of the file: --dtype stays int8")
        if a.packed_frame is not None:
            try:
                parts = [int(x) for x in a.packed_frame.split(":")]
                frame, first = parts[0], (parts[1] if len(parts) > 1 else 0)
                ok = len(parts) <= 2 and frame in (1, 2, 4, 8, 16) and \
                    0 <= first <= frame - (2 if a.iq is not None and frame > 1 else 1)
            except ValueError:
                ok = False
            if not ok:
                ap.error("--packed-frame takes F[:FIRST] with F one of 1, 2, 4, 8, 16 and the kept fields inside the frame")
        if a.packed_peak is not None and not ((1 << a.packed) - 1 <= a.packed_peak <= 127):
            ap.error("--packed-peak takes the largest level in LSB, %d .. 127" % ((1 << a.packed) - 1))
    if a.condition is not None and a.iq_requantize is not None:
        ap.error("--condition stands where --iq-requantize does: not both")
    if a.condition is not None and not (a.condition in (-1.0, 0.0) or 1.0 <= a.condition <= 16.0):
        ap.error("--condition takes the blanking threshold in units of the rms, 1 .. 16, or 0 for no blanking")
    if a.iq_requantize is not None and a.iq is None:
        ap.error("--iq-requantize prepares an I/Q file for the converter: it needs --iq")
    if a.iq_requantize is not None and not (a.iq_requantize == -1.0 or 0.0 < a.iq_requantize <= 127.0):
        ap.error("--iq-requantize takes the rms of the int8 record in LSB, above 0 and at most 127")
    if a.iq is not None and a.correlator_bank is not None:
        ap.error("--correlator-bank replays from the record file, which --iq converts on the way in: not both")
    taps = None
    if a.correlator_bank is not None:
        try:
            lo, hi, step = (float(x) for x in a.correlator_bank.split(":"))
            taps = lo + step * np.arange(int(np.floor((hi - lo) / step + 1e-9)) + 1)
        except (ValueError, ZeroDivisionError):
            taps = None
        if taps is None or not (1 <= taps.size <= 64) or not np.all(np.isfinite(taps)):
            ap.error("--correlator-bank takes LO:HI:STEP in chips with 1 .. 64 taps, e.g. --correlator-bank=-1:1:0.25")
    print('\nWelcome to:  softGNSS on MI355X\n')
    settings = initialize.Settings()
    settings.fileName = a.fileName
    for name, val in (("samplingFreq", a.fs), ("IF", a.IF), ("msToProcess", a.ms), ("numberOfChannels", a.channels),
                      ("skipNumberOfBytes", a.skip), ("lockDetector", True if a.lock_detector else None),
                      ("acqCoherentMs", a.acq_coherent_ms), ("acqBlocks", a.acq_blocks),
                      ("acqNonCoherent", True if a.acq_noncoh else None),
                      ("iqRecord", True if a.iq is not None else None), ("iqQFirst", True if a.iq == "qi" else None),
                      ("dataType", a.dtype),
                      ("iqRequantize", True if a.iq_requantize is not None else None),
                      ("iqTargetRms", a.iq_requantize if a.iq_requantize is not None and a.iq_requantize > 0 else None),
                      ("frontEndConditioning", True if a.condition is not None else None),
                      ("condBlankFactor", a.condition if a.condition is not None and a.condition >= 0 else None),
                      ("packedBits", a.packed), ("packedEncoding", a.packed_encoding),
                      ("packedLsbFirst", True if a.packed_lsb_first else None), ("packedFrame", frame),
                      ("packedFirst", first), ("packedPeak", a.packed_peak),
                      ("decimation", decim), ("decimTaps", decim_taps), ("decimBandwidth", a.decimate_bandwidth),
                      ("resampleUp", up), ("resampleDown", down), ("resampTaps", resamp_taps),
                      ("resampCutoff", a.resample_cutoff),
                      ("interferenceMitigation", True if a.notch is not None else None),
                      ("notchThresholdDb", a.notch if a.notch is not None and a.notch >= 0 else None)):
        if val is not None:
            setattr(settings, name, val)
    if settings.resampleUp:
        real = settings._prepared_settings()
        print('Resampled by %d/%d: read as a real record at %.6f Msps, IF %.6f MHz'
              % (settings.resampleUp, settings.resampleDown, real.samplingFreq / 1e6, real.IF / 1e6))
    elif settings.decimation:
        real = settings._prepared_settings()
        print('Decimated by %d: read as a real record at %.6f Msps, IF %.6f MHz'
              % (settings.decimation, real.samplingFreq / 1e6, real.IF / 1e6))
    elif settings.iqRecord:
        real = settings.realEquivalent()
        print('I/Q record at %.6f Msps, carrier at %+.6f MHz: read as a real record at %.6f Msps, IF %.6f MHz'
              % (settings.samplingFreq / 1e6, settings.IF / 1e6, real.samplingFreq / 1e6, real.IF / 1e6))
    if not a.no_probe:
        print('Probing data "%s"...' % settings.fileName)
        p = probe_iq(settings) if settings.iqRecord or settings.packedBits or settings.decimation \
            or settings.resampleUp else settings.probeData()
        if p is not None:
            k = int(np.argmax(p["Pxx"]))
            print('  %d Welch segments, spectral peak at %.3f MHz, samples within [%d, %d]'
                  % (p["segments"], p["f_MHz"][k], p["hist_edges"][np.flatnonzero(p["hist"])[0]],
                     p["hist_edges"][np.flatnonzero(p["hist"])[-1]] + 1))
    acq, trk, nav = settings.postProcessing()
    if taps is not None and trk is not None and trk.has_results():
        with open(settings.fileName, 'rb') as fid:
            bank = trk.replay(fid, taps)
        print('Correlator bank (%d taps, mean envelope over the run, %.3f ms on the GPU):' % (taps.size, bank.kernel_ms))
        bank.show()
    if nav is not None and nav._solutions is not None:
        sol = nav.solutions[0]
        ok = np.isfinite(sol.X)
        print('  %d position fixes; mean latitude %.6f deg, longitude %.6f deg, height %.1f m (UTM zone %d)'
              % (int(ok.sum()), np.nanmean(sol.latitude), np.nanmean(sol.longitude), np.nanmean(sol.height),
                 int(sol.utmZone)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
