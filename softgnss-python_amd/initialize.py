"""Settings / Result / TruePosition with the reference's names (reference initialize.py:20-185).

The three helpers the hot path calls - generateCAcode, makeCaTable, calcLoopCoef - are answered
by libsgx.so's exact host routines (include/sgx.h), not by Python arithmetic.
"""
import ctypes as C
import datetime
import os

import numpy as np

from . import _native, frontend


class Result(object):
    """Base of AcquisitionResult / TrackingResult (reference initialize.py:20-46)."""

    def __init__(self, settings):
        self._settings = settings
        self._results = None
        self._channels = None

    @property
    def settings(self):
        return self._settings

    def _materialize(self):
        """Hook of the subclasses: results that are still queued on the GPU, or not yet packed into record arrays, are
        brought in before anybody looks (the reference computes everything eagerly; so does this class by default)."""

    @property
    def channels(self):
        self._materialize()
        assert isinstance(self._channels, np.recarray)
        return self._channels

    @property
    def results(self):
        self._materialize()
        assert isinstance(self._results, np.recarray)
        return self._results

    @results.setter
    def results(self, records):
        assert isinstance(records, np.recarray)
        self._results = records

    def plot(self):
        pass


def _pyplot(what):
    """matplotlib.pyplot, or None (with a one-line notice) where matplotlib is not installed: a script that calls
    plot() like the reference's postProcessing does keeps running."""
    try:
        import matplotlib.pyplot as plt
        return plt
    except ImportError:
        print("   (%s: matplotlib is not installed, nothing drawn)" % what)
        return None


class TruePosition(object):
    """E/N/U holder (reference initialize.py:49-77)."""

    def __init__(self):
        self.E = self.N = self.U = None


# attribute -> default, the receiver configuration of reference initialize.py:85-173 (same names, same values)
_DEFAULTS = (
    ("msToProcess", 37000.0), ("numberOfChannels", 8), ("skipNumberOfBytes", 0),
    ("fileName", 'GPSdata-DiscreteComponents-fs38_192-if9_55.bin'), ("dataType", 'int8'),
    ("IF", 9548000.0), ("samplingFreq", 38192000.0), ("codeFreqBasis", 1023000.0), ("codeLength", 1023),
    ("skipAcquisition", False), ("acqSearchBand", 14.0), ("acqThreshold", 2.5),
    ("dllDampingRatio", 0.7), ("dllNoiseBandwidth", 2.0), ("dllCorrelatorSpacing", 0.5),
    ("pllDampingRatio", 0.7), ("pllNoiseBandwidth", 25.0),
    ("navSolPeriod", 500.0), ("elevationMask", 10.0), ("useTropCorr", True), ("plotTracking", True),
)

# the lock detector the reference leaves as a hook (tracking.py:276-278): TrackingResult.quality and, with lockDetector,
# status '-' for every channel it declares lost ("C/N0 and lock detector")
_LOCK_DEFAULTS = (
    ("lockDetector", False),        # run it inside track() and mark lost channels '-'
    ("cnoInterval", 20.0),          # ms per C/N0 window
    ("cnoThreshold", 25.0),         # dB-Hz a window must reach to pass
    ("carrLockThreshold", 0.85),    # cos(2 phi) a window must reach to pass
    ("maxLockFail", 25),            # the fail counter (fail +1, pass -1, not below 0) at which a channel is lost
)

# the coarse search postProcessing() asks for (AcquisitionResult.acquire; INTEGRATION.md, "Coherent acquisition"): the
# reference's is 2 one-millisecond blocks on a 500 Hz grid
_ACQ_DEFAULTS = (
    ("acqCoherentMs", 1),           # ms summed coherently per window
    ("acqBlocks", 2),               # windows
    ("acqNonCoherent", False),      # sum |corr|^2 over the windows instead of keeping the larger one
    ("acqBinStep", None),           # Doppler step in Hz; None: 500 / acqCoherentMs
)

# bit-aligned coherent tracking of weak signals (TrackingResult.track; INTEGRATION.md, "Coherent tracking"): after a pull-in
# with the reference's 1 ms loops the filters are updated once per trackCoherentMs blocks, aligned with the bit edge
_COH_TRACK_DEFAULTS = (
    ("trackCoherentMs", 1),         # ms per loop update behind the pull-in: 1 (the reference), 2, 4, 5, 10 or 20
    ("trackPullInMs", 1000),        # blocks tracked with the reference's loops first; the bit edge is found over them
    ("trackHandOverMs", 100),       # blocks whose NCO values are averaged where the coherent loops take over
    ("cohPllNoiseBandwidth", 3.0),  # Hz, nominal (calcLoopCoef's k = 0.25 makes the loop about twice as wide)
    ("cohDllNoiseBandwidth", 1.0),  # Hz
)

# strong-signal cancellation behind tracking (TrackingResult.cancel; INTEGRATION.md, "Strong-signal cancellation"): the
# channels tracked at a high C/N0 are subtracted from the record, and what they hid is searched for and tracked on the result
_CANCEL_DEFAULTS = (
    ("strongSignalCancellation", False),   # postProcessing() cancels, searches again and tracks what that finds
    ("cancelCNoThreshold", 60.0),          # dB-Hz: a channel whose medianCNo reaches it is cancelled
    ("cancelSmoothMs", 1),                 # blocks an amplitude pair is averaged over, odd, 1 .. 41
)


class Settings(frontend.FrontEnd):
    """Receiver configuration; attribute names and defaults of reference initialize.py:81-173.  The stages between a record
    file and acquisition, and their settings, are frontend.py's."""

    c = property(lambda self: 299792458.0, doc="speed of light, m/s (read-only, initialize.py:170)")
    startOffset = property(lambda self: 68.802, doc="initial travel-time guess, ms (read-only, initialize.py:172)")

    def __init__(self):
        for name, value in _DEFAULTS + _LOCK_DEFAULTS + _ACQ_DEFAULTS + _COH_TRACK_DEFAULTS + _CANCEL_DEFAULTS + frontend.DEFAULTS:
            setattr(self, name, value)
        self.acqSatelliteList = range(1, 33)      # PRN indices 0..31 are searched (acquisition.py:103)
        self.truePosition = TruePosition()

    @property
    def samplesPerCode(self):
        n = C.c_int64(0)
        st = _native.settings_struct(self)
        _native.check(_native.lib().sgx_samples_per_code(C.byref(st), C.byref(n)))
        return int(n.value)

    def makeCaTable(self):
        """float64[32, samplesPerCode] sampled C/A codes (reference initialize.py:188-231)."""
        st = _native.settings_struct(self)
        out = np.empty((32, self.samplesPerCode))
        _native.check(_native.lib().sgx_make_ca_table(C.byref(st), out.ctypes.data_as(C.c_void_p)))
        return out

    def generateCAcode(self, prn):
        """float64[1023] of +-1 for PRN index 0..31 (reference initialize.py:234-302)."""
        assert prn in range(0, 32)
        out = np.empty(1023)
        _native.check(_native.lib().sgx_generate_ca_code(int(prn), out.ctypes.data_as(C.c_void_p)))
        return out

    @staticmethod
    def calcLoopCoef(LBW, zeta, k):
        """(tau1, tau2) of the loop filter (reference initialize.py:304-328)."""
        t1 = C.c_double(0)
        t2 = C.c_double(0)
        _native.check(_native.lib().sgx_calc_loop_coef(float(LBW), float(zeta), float(k), C.byref(t1),
                                                       C.byref(t2)))
        return t1.value, t2.value

    def probeData(self, fileNameStr=None, device=None):
        """Raw-data information of reference initialize.py:330-417 for the first 10 code periods of the record:
        time-domain samples, Welch power spectral density (16384-point periodic Hamming window, 1024 overlap) and
        the histogram.  The numbers come from sgx_probe_stats on the GPU; they are returned as a dict (keys
        timeScale_ms, timeData, f_MHz, Pxx, hist, hist_edges, segments) and kept in self.probe.  The three
        panels are drawn like the reference does when matplotlib is installed.  `fileNameStr` may also be a
        DeviceSignal (a window of a record already resident in HBM)."""
        from . import engine
        from .record import DeviceSignal
        if fileNameStr is None:
            fileNameStr = self.fileName
        samplesPerCode = self.samplesPerCode
        n_want = 10 * samplesPerCode
        ctx = engine.get_context(self, device)
        if isinstance(fileNameStr, DeviceSignal):
            sig = fileNameStr
            n = min(n_want, sig.length)
            head = sig.record.download(sig.offset + 1, max(0, min(samplesPerCode // 50, n) - 1))
            f, pxx, hist, nseg = ctx.probe_stats(sig.record, sig.offset, n, self.samplingFreq / 1000000.0)
        else:
            if not isinstance(fileNameStr, str):
                raise TypeError('File name must be a string')
            try:
                with open(fileNameStr, 'rb') as fid:
                    fid.seek(self.skipNumberOfBytes, 0)
                    data = np.fromfile(fid, self.dataType, n_want)
            except IOError as e:
                print('Unable to read file "%s": %s' % (fileNameStr, e))
                return None
            rec = ctx.upload(data)
            try:
                f, pxx, hist, nseg = ctx.probe_stats(rec, 0, data.size, self.samplingFreq / 1000000.0)
            finally:
                rec.free()
            head = data[1:samplesPerCode // 50]
        timeScale = np.arange(0, 0.005, 1 / self.samplingFreq)
        self.probe = dict(timeScale_ms=1000 * timeScale[1:samplesPerCode // 50], timeData=head,
                          f_MHz=f, Pxx=pxx, hist=hist, hist_edges=np.arange(-128, 128), segments=nseg)
        try:
            import matplotlib.pyplot as plt
        except ImportError:
            return self.probe
        plt.figure(100)
        plt.clf()
        plt.subplot(2, 2, 1)
        if head is not None:
            plt.plot(self.probe["timeScale_ms"], head)
        plt.grid()
        plt.title('Time domain plot')
        plt.xlabel('Time (ms)')
        plt.ylabel('Amplitude')
        plt.subplot(2, 2, 2)
        plt.semilogy(f, pxx)
        plt.grid()
        plt.title('Frequency domain plot')
        plt.xlabel('Frequency (MHz)')
        plt.ylabel('Magnitude')
        plt.subplot(2, 1, 2)
        plt.bar(np.arange(-128, 127), hist, width=1.0, align='edge')
        plt.grid(True)
        plt.title('Histogram')
        plt.xlabel('Bin')
        plt.ylabel('Number in bin')
        return self.probe

    def _acquire_and_track(self, results, acq_source, track_source):
        """postProcessing()'s acquire -> preRun -> track.  results: the settings the results carry (self, or
        realEquivalent()); the sources: an ndarray and the open record file, or a DeviceSignal and a DeviceFile.  Returns
        (acqResults, trackResults), trackResults None where no satellite was found."""
        from . import acquisition, tracking
        print('   Acquiring satellites...')
        acqResults = acquisition.AcquisitionResult(results)
        acqResults.acquire(acq_source, n_blocks=int(self.acqBlocks), noncoh=bool(self.acqNonCoherent),
                           coherent_ms=int(self.acqCoherentMs), bin_step_hz=self.acqBinStep)
        if not np.any(acqResults.carrFreq):
            print('No GNSS signals detected, signal processing finished.')
            return acqResults, None
        acqResults.preRun()
        acqResults.showChannelStatus()
        trackResults = tracking.TrackingResult(acqResults)
        start = datetime.datetime.now()
        print('   Tracking started at %s' % start.strftime('%X'))
        trackResults.track(track_source)
        self.lastTrackingSeconds = (datetime.datetime.now() - start).total_seconds()
        print('   Tracking is over (elapsed time %s s)' % self.lastTrackingSeconds)
        if self.lockDetector and trackResults.has_results():
            trackResults.showTrackingQuality()
        if self.strongSignalCancellation and trackResults.has_results():
            trackResults = self._cancel_strong(results, acqResults, trackResults, track_source)
        return acqResults, trackResults

    def _cancel_strong(self, results, acqResults, trackResults, track_source):
        """strongSignalCancellation, behind tracking: every channel whose medianCNo reaches cancelCNoThreshold is cancelled
        (TrackingResult.cancel), the PRNs that are not tracked are searched again on the cleaned record with this call's
        acquisition settings, what that finds is tracked on the cleaned record in the free channels, and the rows join the
        others (TrackingResult.join).  Sample positions are those of the record as it was.  Returns the tracking results
        that go on to navigation: the joined ones, or trackResults where nothing was cancelled or nothing new found."""
        from . import acquisition, tracking
        from .record import DeviceFile, DeviceSignal
        quality = trackResults.quality
        rows = [j for j in range(len(quality)) if quality[j].medianCNo >= float(self.cancelCNoThreshold)]
        if not rows:
            print('   No channel reaches %.1f dB-Hz: nothing is cancelled' % float(self.cancelCNoThreshold))
            return trackResults
        nch, n = int(results.numberOfChannels), results.samplesPerCode
        tracked = [int(p) for p in trackResults.results.PRN]
        print('   Cancelling PRN %s (median C/N0 %s dB-Hz)...' % (
            ", ".join("%d" % tracked[j] for j in rows), ", ".join("%.1f" % quality[j].medianCNo for j in rows)))
        skip, own = int(results.skipNumberOfBytes), None
        if not isinstance(track_source, DeviceFile):     # the record file: the bytes the search and both trackings read
            start = (skip // 4096) * 4096
            need = skip - start + max(results.acquisitionLength() + n, int(results.msToProcess) * (n + 2) + 2 * n)
            name = getattr(track_source, 'name', None)
            if isinstance(name, (str, bytes)) and os.path.isfile(name):
                need = min(need, os.path.getsize(name) - start)
            own = trackResults._window(track_source, start, need)
            track_source = DeviceFile(own, start)
        cleaned = None
        try:
            cleaned = trackResults.cancel(track_source, rows, smooth=int(self.cancelSmoothMs))
            print('   %d channels cancelled in %.3f ms on the GPU, %d samples clipped' % (len(rows), cleaned.kernel_ms,
                                                                                     cleaned.clipped))
            free = nch - len(tracked)
            left = [p for p in range(len(results.acqSatelliteList)) if p + 1 not in tracked]
            # the search starts one code period behind skipNumberOfBytes: every cancelled channel's first block starts in
            # front of that, so no sample of the window still holds a strong signal; a code phase found there holds one
            # period earlier, where tracking starts (the loops pull in the fraction of a sample it may be off)
            at = skip - cleaned.file_offset
            if len(cleaned.record) - (at + n) >= results.acquisitionLength():
                at += n
            if free < 1 or not left or at < 0:
                return trackResults
            again = acquisition.AcquisitionResult(results)
            again.acquire(DeviceSignal(cleaned.record, at, min(results.acquisitionLength(), len(cleaned.record) - at)),
                          n_blocks=int(self.acqBlocks), noncoh=bool(self.acqNonCoherent), coherent_ms=int(self.acqCoherentMs),
                          bin_step_hz=self.acqBinStep, prn_indices=left)
            found = int(np.sum(again.carrFreq > 0))
            if not found:
                print('   The cleaned record shows no further satellite')
                return trackResults
            again.preRun()
            table = again.channels
            for i in range(min(free, found), nch):       # (the free channels only: the strongest of what was found)
                table[i].PRN, table[i].acquiredFreq, table[i].codePhase, table[i].status = 0, 0.0, 0.0, '-'
            print('   Found on the cleaned record: PRN %s' % ", ".join("%d" % p for p in table.PRN if p))
            more = tracking.TrackingResult(again)
            more.track(cleaned)
            if not more.has_results():
                return trackResults
            for p in (int(q) - 1 for q in table.PRN if q):
                for name in ("carrFreq", "codePhase", "peakMetric"):
                    acqResults.results[name][p] = again.results[name][p]
            joined = trackResults.join(more)
            if self.lockDetector:
                joined.showTrackingQuality()
            return joined
        finally:
            if cleaned is not None:
                cleaned.record.free()
            if own is not None:
                own.free()

    def _resident_processing(self, name):
        """postProcessing()'s acquire -> preRun -> track on a record that _prepared_record uploads once and prepares on the
        GPU; both stages read the prepared record where it lies.  The results carry _prepared_settings(): positions
        (codePhase, absoluteSample, skipNumberOfBytes) are samples of the prepared record; which byte of the file a sample
        is made of, stage by stage, is _file_range()'s to say."""
        from .record import DeviceFile, DeviceSignal
        real = self._prepared_settings()
        n = real.samplesPerCode
        skip = int(real.skipNumberOfBytes)
        need = skip + max(real.acquisitionLength(), int(self.msToProcess) * (n + 2) + 2 * n)
        if self.iqRecord:
            need += need % 2                         # (whole pairs; with decimation: whole groups of D pairs)
        mitigating = self.interferenceMitigation or self.sweptMitigation
        with self._prepared_record(name, 0, need, skip if mitigating else None, verbose=True) as rec:
            window = DeviceSignal(rec, skip, min(real.acquisitionLength(), max(0, len(rec) - skip)))
            return self._acquire_and_track(real, window, DeviceFile(rec))

    def acquisitionLength(self):
        """Samples postProcessing() reads for acquisition: 11 ms (the fine search needs codePhase + 10 ms), or all the
        coarse search's windows, acqCoherentMs x acqBlocks ms, where that is longer."""
        return max(11, int(self.acqCoherentMs) * int(self.acqBlocks)) * self.samplesPerCode

    def postProcessing(self, fileNameStr=None):
        """acquire -> preRun -> track -> postNavigate on a record file: the call sequence of reference
        initialize.py:420-515 without the plots and without the .npy cache of the tracking results.
        Returns (acqResults, trackResults, navResults); navResults.solutions is unset when the record is too short
        or too few satellites carry ephemerides, as in the reference."""
        print('Starting processing...')
        name = self.fileName if not fileNameStr else fileNameStr
        if not isinstance(name, str):
            raise TypeError('File name must be a string')
        if self.skipAcquisition:
            # (the reference then reads acqResults before anything assigned it: NameError, initialize.py:476,490)
            raise ValueError('skipAcquisition is set, but there are no acquisition results to reuse: '
                             'postProcessing() always acquires (initialize.py:476-490)')
        if self.interferenceMitigation or self.sweptMitigation or any(stage.on(self) for stage in frontend.STAGES):
            acqResults, trackResults = self._resident_processing(name)
            if trackResults is None:
                return acqResults, None, None
            return self._navigate(acqResults, trackResults)
        with open(name, 'rb') as fid:
            fid.seek(self.skipNumberOfBytes, 0)
            data = np.fromfile(fid, self.dataType, self.acquisitionLength())
            acqResults, trackResults = self._acquire_and_track(self, data, fid)
        if trackResults is None:
            return acqResults, None, None
        return self._navigate(acqResults, trackResults)

    @staticmethod
    def _navigate(acqResults, trackResults):
        """The tail of postProcessing(): the navigation solution from the tracking results."""
        from . import postNavigation
        if not trackResults.has_results():   # (the reference's short-read exit: results were not set, tracking.py:159-163)
            return acqResults, trackResults, None
        print('   Calculating navigation solutions...')
        navResults = postNavigation.NavigationResult(trackResults)
        navResults.postNavigate()
        print('   Processing is complete for this data block')
        return acqResults, trackResults, navResults
