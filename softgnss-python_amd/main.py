"""The reference's main.py (banner, probeData, postProcessing) for this engine:

    python -m softgnss-python_amd.main record.bin [--fs 38192000 --IF 9548000 --ms 37000 --channels 8 --skip 0]
                                                  [--lock-detector] [--acq-coherent-ms T --acq-blocks M --acq-noncoh]
                                                  [--correlator-bank LO:HI:STEP] [--notch[=THRESHOLD_DB]] [--dtype int8]
                                                  [--excise[=THRESHOLD] --excise-segment N]
                                                  [--cancel-strong[=DBHZ] --cancel-smooth MS]
                                                  [--track-coherent-ms T --track-pull-in-ms P --coh-pll-bw HZ --coh-dll-bw HZ]
%s

Prints the channel table, the tracking time (with --lock-detector: each channel's C/N0, carrier lock and the time it
was lost, lost channels leaving the navigation) and, when the record is long enough (36 s, four satellites with
ephemerides), the mean position fix.  --correlator-bank=-1:1:0.25 replays the tracked channels at those code offsets
(chips) and prints each channel's mean correlation envelope per tap, normalised to its maximum.  --notch looks for
continuous-wave lines in the record's spectrum (8 dB above the local median, or --notch=THRESHOLD_DB), filters them out on
the GPU before acquisition and tracking, and prints the lines it removed.  --excise removes swept (chirp) interference in
front of that: every segment of 256 samples (or --excise-segment N, a power of two in 64 .. 1024) loses the bins of its
spectrum that stand 8 times (or --excise=THRESHOLD times) above the mean of its other bins; it prints the share of the
time-frequency cells it cut and the samples it clipped.  --cancel-strong works behind tracking: every channel tracked at a
median C/N0 of 60 dB-Hz or more (or --cancel-strong=DBHZ) is rebuilt from its tracking results and subtracted from the record
(one amplitude per block, or averaged over --cancel-smooth MS blocks, odd, 1 .. 41), the satellites that are not tracked are
searched for again on the cleaned record and those found are tracked there in the free channels; they join the others for
navigation.  --track-coherent-ms 20 keeps weak signals: after --track-pull-in-ms ms with the 1 ms loops (over which each
channel's bit edge is found) both loops are updated once per 20 ms from sums aligned with the navigation bits.
%s

--monitor looks at the whole prepared record before anything else runs: per 100 ms (or --monitor=SLICE_MS) one Welch spectrum
and the exact statistics of the samples, on the GPU in one pass.  It prints a line per event - a spectral line --notch would
find, with the time it is first and last seen and how far it stands over the floor - and per slice whose kurtosis or share of
clipped samples stands out of the record's own slices (pulsed interference); --monitor-out FILE.npz saves the arrays.  With
--notch, --notch-whole-record designs the notch from the largest value every bin of that spectrum takes anywhere in the record
instead of from its first 10 ms: a jammer that switches on later is removed too."""
from __future__ import print_function

import argparse

import numpy as np

from . import initialize
from .frontend import DTYPE_HELP, STAGES


def _synopsis(flag, keywords):
    value = keywords.get("metavar") or "|".join(keywords.get("choices", ()))
    return flag + ("[=%s]" % value if keywords.get("nargs") == "?" else " " + value if value else "")


# the record front end says how its stages are spelled: a line of the synopsis and a paragraph per entry of frontend.STAGES
__doc__ = __doc__ % ("\n".join(" " * 50 + "[%s]" % " ".join(_synopsis(*opt) for opt in stage.options) for stage in STAGES),
                     "\n".join(stage.usage for stage in STAGES))


def probe_iq(settings):
    """probeData() of a file the record front end prepares: its first 10 code periods, as the real int8 record they become."""
    from .record import DeviceSignal
    real = settings._prepared_settings()
    with settings._prepared_record(settings.fileName, int(real.skipNumberOfBytes), 10 * real.samplesPerCode) as rec:
        return real.probeData(DeviceSignal(rec))


def monitor_file(settings, out=None):
    """--monitor: monitorRecord() of the prepared record postProcessing will read, from skipNumberOfBytes on; a line per
    event and per flagged slice; the arrays to `out` (.npz) where that is given.  Returns the info."""
    real = settings._prepared_settings()
    n, skip = real.samplesPerCode, int(real.skipNumberOfBytes)
    need = skip + max(real.acquisitionLength(), int(settings.msToProcess) * (n + 2) + 2 * n)
    if settings.iqRecord:
        need += need % 2
    print('Monitoring "%s"...' % settings.fileName)
    with settings._prepared_record(settings.fileName, 0, need) as rec:
        info = real.monitorRecord(rec, min(skip, len(rec)))
    settings.lastMonitor = info
    seen = info["waterfall"]
    print('  %d slices of %.1f ms, %d Welch segments each' % (len(seen.n_segments), info["slice_ms"],
                                                              int(seen.n_segments[0])))
    for f_hz, w_hz, first_ms, last_ms, peak_db in info["events"]:
        print('  Line at %.4f MHz (%.1f kHz wide) from %.0f to %.0f ms, %.1f dB over the floor'
              % (f_hz / 1e6, w_hz / 1e3, first_ms, last_ms, peak_db))
    for j in info["pulsed"]:
        print('  Slice at %.0f ms stands out: excess kurtosis %+.3f, %.4f %% of the samples clipped'
              % (j * info["slice_ms"], seen.kurtosis[j], 100.0 * seen.clip_share[j]))
    if not info["events"] and not info["pulsed"]:
        print('  Nothing stands out')
    if out is not None:
        np.savez(out, slice_ms=info["slice_ms"], events=np.array(info["events"], dtype=np.float64).reshape(-1, 5),
                 pulsed=np.array(info["pulsed"], dtype=np.int64), **seen.arrays())
    return info


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
    ap.add_argument("--track-coherent-ms", type=int, default=None, metavar="T",
                    help="tracking: behind the pull-in, update the loops once per T ms (2, 4, 5, 10 or 20), aligned with the "
                         "navigation bit - keeps signals the 1 ms loops lose (below ~30 dB-Hz)")
    ap.add_argument("--track-pull-in-ms", type=int, default=None, metavar="P",
                    help="with --track-coherent-ms: ms tracked with the 1 ms loops first, over which the bit edge is found "
                         "(default: Settings.trackPullInMs, 1000; at least 220)")
    ap.add_argument("--coh-pll-bw", type=float, default=None, metavar="HZ",
                    help="with --track-coherent-ms: nominal PLL noise bandwidth of the coherent loop (default 3)")
    ap.add_argument("--coh-dll-bw", type=float, default=None, metavar="HZ",
                    help="with --track-coherent-ms: DLL noise bandwidth of the coherent loop (default 1)")
    ap.add_argument("--correlator-bank", default=None, metavar="LO:HI:STEP",
                    help="after tracking, replay every channel at code offsets LO .. HI (chips, at most 64 taps) and "
                         "print the mean envelope per tap (a negative LO needs the = form: --correlator-bank=-1:1:0.25)")
    ap.add_argument("--notch", nargs="?", type=float, const=-1.0, default=None, metavar="THRESHOLD_DB",
                    help="excise narrowband interference before acquisition: notch out the spectral lines that stand "
                         "THRESHOLD_DB (default: Settings.notchThresholdDb, 8) above the local median")
    ap.add_argument("--excise", nargs="?", type=float, const=-1.0, default=None, metavar="THRESHOLD",
                    help="excise swept (chirp) interference before the notch and acquisition: cut the bins of every short "
                         "segment that stand THRESHOLD times (default: Settings.exciseThreshold, 8) above the mean of its "
                         "other bins")
    ap.add_argument("--excise-segment", type=int, default=None, metavar="N",
                    help="with --excise: the segment length, a power of two in 64 .. 1024 (default: Settings.exciseSegment, "
                         "256)")
    ap.add_argument("--cancel-strong", nargs="?", type=float, const=-1.0, default=None, metavar="DBHZ",
                    help="after tracking, cancel every channel whose median C/N0 reaches DBHZ (default: "
                         "Settings.cancelCNoThreshold, 60), search the cleaned record for the satellites that are not "
                         "tracked and track what that finds in the free channels")
    ap.add_argument("--cancel-smooth", type=int, default=None, metavar="MS",
                    help="with --cancel-strong: average each block's amplitude over MS blocks, odd, 1 .. 41 (default: "
                         "Settings.cancelSmoothMs, 1)")
    ap.add_argument("--monitor", nargs="?", type=float, const=-1.0, default=None, metavar="SLICE_MS",
                    help="monitor the whole record first: a spectrum and sample statistics per SLICE_MS ms (default: "
                         "Settings.monitorSliceMs, 100), a line printed per event and per slice that stands out")
    ap.add_argument("--monitor-out", default=None, metavar="FILE.npz", help="with --monitor: save the monitor's arrays")
    ap.add_argument("--notch-whole-record", action="store_true",
                    help="with --notch: design the notch from the spectrum of the whole record, not of its first 10 ms")
    ap.add_argument("--dtype", default=None, help=DTYPE_HELP)
    dests = [[ap.add_argument(flag, **keywords).dest for flag, keywords in stage.options] for stage in STAGES]
    a = ap.parse_args(argv)
    taps = None
    if a.correlator_bank is not None:
        try:
            lo, hi, step = (float(x) for x in a.correlator_bank.split(":"))
            taps = lo + step * np.arange(int(np.floor((hi - lo) / step + 1e-9)) + 1)
        except (ValueError, ZeroDivisionError):
            taps = None
        if taps is None or not (1 <= taps.size <= 64) or not np.all(np.isfinite(taps)):
            ap.error("--correlator-bank takes LO:HI:STEP in chips with 1 .. 64 taps, e.g. --correlator-bank=-1:1:0.25")
    if a.notch_whole_record and a.notch is None:
        ap.error("--notch-whole-record says what --notch designs its filter from: it needs --notch")
    if a.excise_segment is not None and a.excise is None:
        ap.error("--excise-segment says how --excise cuts the record: it needs --excise")
    if a.excise is not None and not (a.excise == -1.0 or (np.isfinite(a.excise) and a.excise >= 1.0)):
        ap.error("--excise takes the threshold, a factor of at least 1")
    if a.excise_segment is not None and not (64 <= a.excise_segment <= 1024 and a.excise_segment & (a.excise_segment - 1) == 0):
        ap.error("--excise-segment takes a power of two in 64 .. 1024")
    if a.cancel_smooth is not None and a.cancel_strong is None:
        ap.error("--cancel-smooth says how --cancel-strong forms its amplitudes: it needs --cancel-strong")
    if a.cancel_strong is not None and not (a.cancel_strong == -1.0 or np.isfinite(a.cancel_strong)):
        ap.error("--cancel-strong takes the C/N0 threshold in dB-Hz")
    if a.cancel_smooth is not None and not (1 <= a.cancel_smooth <= 41 and a.cancel_smooth % 2 == 1):
        ap.error("--cancel-smooth takes an odd number of blocks in 1 .. 41")
    if a.track_coherent_ms is not None and a.track_coherent_ms not in (1, 2, 4, 5, 10, 20):
        ap.error("--track-coherent-ms takes 1, 2, 4, 5, 10 or 20")
    if a.track_coherent_ms in (None, 1) and not (a.track_pull_in_ms is None and a.coh_pll_bw is None and a.coh_dll_bw is None):
        ap.error("--track-pull-in-ms, --coh-pll-bw and --coh-dll-bw describe the coherent loops: they need --track-coherent-ms")
    if a.track_pull_in_ms is not None and a.track_pull_in_ms < 220:
        ap.error("--track-pull-in-ms takes at least 220 ms (the bit edge is found over them)")
    if (a.coh_pll_bw is not None and not a.coh_pll_bw > 0) or (a.coh_dll_bw is not None and not a.coh_dll_bw > 0):
        ap.error("--coh-pll-bw and --coh-dll-bw take a bandwidth in Hz, above 0")
    if a.monitor_out is not None and a.monitor is None:
        ap.error("--monitor-out saves what --monitor sees: it needs --monitor")
    if a.monitor is not None and not (a.monitor == -1.0 or (np.isfinite(a.monitor) and a.monitor > 0)):
        ap.error("--monitor takes the slice length in ms, above 0")
    settings = initialize.Settings()
    asked = dict(fileName=a.fileName, samplingFreq=a.fs, IF=a.IF, msToProcess=a.ms, numberOfChannels=a.channels,
                 skipNumberOfBytes=a.skip, lockDetector=a.lock_detector or None, acqCoherentMs=a.acq_coherent_ms,
                 acqBlocks=a.acq_blocks, acqNonCoherent=a.acq_noncoh or None, dataType=a.dtype,
                 interferenceMitigation=True if a.notch is not None else None,
                 notchThresholdDb=a.notch if a.notch is not None and a.notch >= 0 else None,
                 notchWholeRecord=a.notch_whole_record or None,
                 sweptMitigation=True if a.excise is not None else None,
                 exciseThreshold=a.excise if a.excise is not None and a.excise >= 1.0 else None,
                 exciseSegment=a.excise_segment,
                 strongSignalCancellation=True if a.cancel_strong is not None else None,
                 cancelCNoThreshold=a.cancel_strong if a.cancel_strong is not None and a.cancel_strong != -1.0 else None,
                 cancelSmoothMs=a.cancel_smooth, trackCoherentMs=a.track_coherent_ms, trackPullInMs=a.track_pull_in_ms,
                 cohPllNoiseBandwidth=a.coh_pll_bw, cohDllNoiseBandwidth=a.coh_dll_bw,
                 monitorSliceMs=a.monitor if a.monitor is not None and a.monitor > 0 else None)
    for stage, names in zip(STAGES, dests):
        given = [val is not None and val is not False for val in (getattr(a, name) for name in names)]
        if given[0]:
            asked.update(stage.settings_from(a, ap.error))
        elif any(given):        # its other options describe what the first one switches on
            ap.error(stage.needs)
    vars(settings).update((name, val) for name, val in asked.items() if val is not None)
    try:                        # what postProcessing would refuse is refused here, before anything is probed or opened
        real = settings._walk()[1]
    except ValueError as e:
        ap.error(str(e))
    on = [stage for stage in STAGES if stage.on(settings)]
    for stage in on:
        if taps is not None and not stage.replays_file:
            ap.error("--correlator-bank replays from the record file, which %s %s on the way in: not both"
                     % (stage.options[0][0], stage.verb))
    print('\nWelcome to:  softGNSS on MI355X\n')
    banner = [stage.announce(settings) for stage in on if stage.announce]
    if banner:                  # the last stage that has a line, and the rate and IF everything else runs at
        print(banner[-1] + ': read as a real record at %.6f Msps, IF %.6f MHz' % (real.samplingFreq / 1e6, real.IF / 1e6))
    if not a.no_probe:
        print('Probing data "%s"...' % settings.fileName)
        p = probe_iq(settings) if on else settings.probeData()
        if p is not None:
            k = int(np.argmax(p["Pxx"]))
            print('  %d Welch segments, spectral peak at %.3f MHz, samples within [%d, %d]'
                  % (p["segments"], p["f_MHz"][k], p["hist_edges"][np.flatnonzero(p["hist"])[0]],
                     p["hist_edges"][np.flatnonzero(p["hist"])[-1]] + 1))
    if a.monitor is not None:
        monitor_file(settings, a.monitor_out)
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
