"""TrackingResult with the reference's interface (reference tracking.py:6-295).

track(fid) reads the part of the record the channels need, puts it in HBM and runs every
channel's DLL/PLL loop in ONE launch of the persistent tracking kernel (sgx_track); the 13
per-millisecond series come back as a record array shaped like the reference's.
"""
from __future__ import print_function

import contextlib
import os

import numpy as np

from . import _native, engine
from .initialize import Result
from .record import DeviceFile

RESULT_DTYPE = [('status', 'S1'), ('absoluteSample', 'object'), ('codeFreq', 'object'),
                ('carrFreq', 'object'), ('I_P', 'object'), ('I_E', 'object'), ('I_L', 'object'),
                ('Q_E', 'object'), ('Q_P', 'object'), ('Q_L', 'object'), ('dllDiscr', 'object'),
                ('dllDiscrFilt', 'object'), ('pllDiscr', 'object'), ('pllDiscrFilt', 'object'),
                ('PRN', 'int64')]   # reference tracking.py:285-293
QUALITY_DTYPE = [('PRN', 'int64'), ('CNo', 'object'), ('carrLock', 'object'), ('lockPass', 'object'),
                 ('lostAtMs', 'int64'), ('medianCNo', 'float64')]
_DT_CODES = {'i1': _native.DT_INT8, 'u1': _native.DT_UINT8, 'i2': _native.DT_INT16, 'u2': _native.DT_UINT16,
             'i4': _native.DT_INT32, 'u4': _native.DT_UINT32, 'i8': _native.DT_INT64, 'u8': _native.DT_UINT64,
             'f2': _native.DT_FLOAT16, 'f4': _native.DT_FLOAT32, 'f8': _native.DT_FLOAT64}   # numpy kind + size -> sgx_track_ex


class ReplayResult(object):
    """What TrackingResult.replay returns: the correlation of every tracked channel at K code offsets, per ms.
    taps float64[K] (chips), PRN int[n_active], I / Q float64[n_active, K, ms] (row order of TrackingResult.results)."""

    def __init__(self, taps, prn, out, kernel_ms=None):
        self.taps = np.array(taps, dtype=np.float64)
        self.PRN = np.array(prn, dtype=np.int64)
        self.I = out[:, :, 0, :]
        self.Q = out[:, :, 1, :]
        self.kernel_ms = kernel_ms   # HIP-event duration of the replay kernel

    def envelope(self):
        """sqrt(I^2 + Q^2), float64[n_active, K, ms]."""
        return np.sqrt(self.I ** 2 + self.Q ** 2)

    def show(self, first_ms=0):
        """ASCII table: per channel, the mean envelope from first_ms on, normalised to its maximum, one line per tap."""
        env = self.envelope()[:, :, first_ms:].mean(axis=2) if self.I.shape[2] > first_ms else self.envelope().mean(axis=2)
        bar = '*=========*=====*==========*==========*'
        print('\n' + bar)
        print('| Channel | PRN | tap chips | envelope |')
        print(bar)
        for c in range(env.shape[0]):
            top = env[c].max()
            for j, d in enumerate(self.taps):
                print('|      %2d | %3d | %8.3f |  %6.3f  |' % (c, int(self.PRN[c]), d, env[c, j] / top if top > 0 else 0.0))
            print(bar)
        print('')


class _Acquired(object):
    """A channel table and its settings: all of an acquisition that a TrackingResult made by join() looks at."""

    def __init__(self, settings, channels):
        self.settings, self.channels = settings, channels


class TrackingResult(Result):
    def __init__(self, acqResult, device=None, verbose=False):
        """verbose: print the reference's progress lines (tracking.py:137-143: one per channel and 50 ms) - after the
        kernel has finished; the GPU is never synchronised every 50 ms to print."""
        self._verbose = verbose
        self._acq = acqResult
        # (a deferred acquisition whose preRun is still to run on the device: the table arrives with the tracking results;
        # anything with .channels and .settings serves as the acquisition)
        self._channels = None if getattr(acqResult, "prerun_queued", False) else acqResult.channels
        self._settings = acqResult.settings
        self._device = device
        self.kernel_ms = None       # HIP-event duration of the tracking kernel
        self._reset()

    def _reset(self):
        """Nothing tracked: where __init__ leaves the object and every track() starts."""
        self._results = None
        self._lazy = None           # (series, active channel numbers): .results is packed on first access
        self.chained = False        # the last track() ran preRun on the device behind a deferred acquisition
        self.series = None          # float64[n_active, 13, ms] in _native.SERIES order
        self._quality = None        # .quality, computed on first access (sgx_track_quality)
        self._lost_rows = ()        # rows of .results the lock detector declared lost inside track() (status '-')
        self._active = []           # channel numbers of the rows of .series
        self._assigned = False      # .results was assigned (the reference's cache path): .quality reads it, not .series
        self.bitEdge = self.coherentStart = self.edgeEnergy = None   # coherent tracking only (Settings.trackCoherentMs > 1)

    def has_results(self):
        """False after the reference's short-read exit (tracking.py:159-163 leaves the results unset) and before track()."""
        return self._results is not None or self._lazy is not None

    def _table(self):
        """The acquisition's channel table, looked at when first needed (a queued search and its preRun end here)."""
        if self._channels is None:
            self._channels = self._acq.channels
        return self._channels

    def _materialize(self):
        self._table()
        if self._lazy is not None:
            series, active = self._lazy
            self._lazy = None
            channel = self._channels
            # reference tracking.py:280-294: one record per ACTIVE channel, each series an object field
            res = np.recarray((len(active),), dtype=RESULT_DTYPE)
            for j, i in enumerate(active):
                res[j].status = channel[i].status
                res[j].PRN = int(channel[i].PRN)
                for k, name in enumerate(_native.SERIES):
                    res[j][name] = series[j, k]
            for j in self._lost_rows:
                res[j].status = '-'
            self._results = res

    @Result.results.setter
    def results(self, records):
        Result.results.fset(self, records)
        self._quality = None
        self._assigned = True

    @property
    def quality(self):
        """C/N0 and lock detector per tracked channel (sgx_track_quality on I_P / Q_P; formulas in INTEGRATION.md):
        a recarray with one row per record of .results - PRN, CNo and carrLock (float64 per cnoInterval window),
        lockPass (bool per window), lostAtMs ((lost window + 1) x cnoInterval, or -1) and medianCNo (median of the
        finite CNo before the loss).  Computed on first access; a new track() starts afresh."""
        if self._quality is None:
            self._quality = self._compute_quality()
        return self._quality

    def _tracked(self, names=_native.SERIES, table=True):
        """What was tracked - from .series, or from an assigned .results (the reference's cache path): (series float64[n,
        k, ms], the row of axis 1 that holds each of `names` - all 13 of .series, only `names` of .results -, PRN per
        channel and, with `table`, each channel's (PRN, acquiredFreq, codePhase) from the acquisition's table)."""
        if self.series is not None and not self._assigned:
            series, row = self.series, {name: _native.SERIES.index(name) for name in names}
            active = list(self._active)
            prn = [int(self._channels[i].PRN) for i in active]
        else:
            res = self.results
            series = np.stack([np.stack([np.asarray(r[name], dtype=np.float64) for name in names]) for r in res]) \
                if len(res) else np.empty((0, len(names), 0))
            row = {name: k for k, name in enumerate(names)}
            prn = [int(p) for p in res.PRN]
            active = None
        if not table:
            return series, row, prn, None
        channel = self._table()
        if active is None:
            active = [i for i in range(len(channel)) if channel[i].PRN != 0][:len(prn)]
            if [int(channel[i].PRN) for i in active] != prn:
                raise ValueError("the results' PRNs are not those of the acquisition's channels: replay() needs each "
                                 "channel's acquiredFreq and codePhase")
        return series, row, prn, [(int(channel[i].PRN), float(channel[i].acquiredFreq), float(channel[i].codePhase))
                                  for i in active]

    def _compute_quality(self):
        settings = self._settings
        params = _native.lock_params(settings)
        series, row, prn, _ = self._tracked(("I_P", "Q_P"), table=False)
        i_p, q_p = series[:, row["I_P"]], series[:, row["Q_P"]]   # rows of the [n, k, ms] array, passed as they lie
        q = np.recarray((len(prn),), dtype=QUALITY_DTYPE)
        if not len(prn):
            return q
        ctx = engine.get_context(settings, self._device)
        cno, carr, ok, lost = ctx.track_quality(i_p, q_p, params)
        W = params.window
        for j in range(len(prn)):
            q[j].PRN = prn[j]
            q[j].CNo = cno[j]
            q[j].carrLock = carr[j]
            q[j].lockPass = ok[j]
            q[j].lostAtMs = (int(lost[j]) + 1) * W if lost[j] >= 0 else -1
            before = cno[j, :lost[j]] if lost[j] >= 0 else cno[j]
            before = before[np.isfinite(before)]
            q[j].medianCNo = float(np.median(before)) if before.size else np.nan
        return q

    def replay(self, fid, taps):
        """Multi-correlator replay (sgx_track_replay): the correlation of every tracked channel at the code offsets
        `taps` (chips, 1 .. 64 of them) for every ms, rebuilt from the recorded absoluteSample / codeFreq / carrFreq -
        taps (-dllCorrelatorSpacing, 0, +dllCorrelatorSpacing) are the early, prompt and late arms themselves.
        fid: the record track() read (open binary file or DeviceFile).  Works after track() and after .results was
        assigned from a cache.  Returns a ReplayResult (.taps, .PRN, .I, .Q, .envelope())."""
        settings = self._settings
        taps = np.atleast_1d(np.asarray(taps, dtype=np.float64))
        series, _, prn, chans = self._tracked()
        if not chans:
            return ReplayResult(taps, prn, np.zeros((0, taps.size, 2, series.shape[2])))
        ctx = engine.get_context(settings, self._device)
        dtype_code, isz = self._data_type()
        first = int(settings.skipNumberOfBytes + min(c[2] for c in chans))
        with self._record(fid, first, lambda: int(series[:, 0, :].max()) - first) as (rec, file_off):
            out = ctx.track_replay(rec, chans, series, taps, rec_file_offset=file_off, data_type=dtype_code)
            kernel_ms = ctx.replay_timing()[0]
        return ReplayResult(taps, prn, out, kernel_ms)

    def cancel(self, fid, rows=None, smooth=1):
        """Strong-signal cancellation (sgx_if_cancel): the signals of tracked channels rebuilt from their recorded blocks
        and prompt sums and subtracted from the record, so that a search of the result finds what they hid.
        fid: the int8 record track() read (open binary file or DeviceFile); rows: the rows of .results to cancel (None:
        all of them, at most 32); smooth: the odd number of blocks, 1 .. 41, each amplitude pair is averaged over.
        Returns a DeviceFile on the NEW record with the input's file_offset - DeviceSignal(result.record, ...) and track()
        take it; its .clipped counts the outputs on the rails, .kernel_ms is the kernel's time.  Works after track() and
        after .results was assigned from a cache."""
        settings = self._settings
        series, _, prn, chans = self._tracked()
        pick = list(range(len(chans or ()))) if rows is None else [int(r) for r in rows]
        if not pick or min(pick) < 0 or max(pick) >= len(chans or ()):
            raise ValueError("cancel() takes rows of .results, 1 .. %d of them: got %r of %d"
                             % (_native.CANCEL_MAX_CHANNELS, pick, len(chans or ())))
        dtype_code, isz = self._data_type()
        if dtype_code != _native.DT_INT8:
            raise TypeError("cancel() rebuilds int8 records, not Settings.dataType %r" % (settings.dataType,))
        chans = [chans[i] for i in pick]
        series = np.ascontiguousarray(series[pick])
        ctx = engine.get_context(settings, self._device)
        first = int(settings.skipNumberOfBytes + min(c[2] for c in chans))
        with self._record(fid, first, lambda: int(series[:, 0, :].max()) - first) as (rec, file_off):
            state = _native.replay_state(settings, chans, series, rec_file_offset=file_off, rec_bytes=len(rec))
            amp = _native.cancel_design(series, state, smooth=smooth)
            out = ctx.if_cancel(rec, chans, series, amp, rec_file_offset=file_off)
            kernel_ms = ctx.cancel_timing()
        cleaned = DeviceFile(out, file_off)
        cleaned.clipped, cleaned.kernel_ms, cleaned.PRN = int(out.clipped), kernel_ms, [c[0] for c in chans]
        return cleaned

    def join(self, other):
        """A TrackingResult that holds this object's rows followed by `other`'s - channels found and tracked later, on a
        cleaned record (Settings.strongSignalCancellation) - over one channel table of numberOfChannels rows: what
        NavigationResult takes.  Both were tracked by track() for the same number of ms."""
        if self.series is None or other.series is None or self.series.shape[2] != other.series.shape[2]:
            raise ValueError("join() takes two results of track() over the same number of ms")
        rows = [self._channels[i] for i in self._active] + [other._channels[i] for i in other._active]
        nch = max(int(self._settings.numberOfChannels), len(rows))
        table = np.rec.fromarrays([np.zeros(nch, dtype='int64'), np.zeros(nch), np.zeros(nch), ['-'] * nch],
                                  names='PRN,acquiredFreq,codePhase,status')
        for i, r in enumerate(rows):
            table[i].PRN, table[i].acquiredFreq, table[i].codePhase = int(r.PRN), float(r.acquiredFreq), float(r.codePhase)
            table[i].status = r.status
        both = TrackingResult(_Acquired(self._settings, table), device=self._device, verbose=self._verbose)
        both.kernel_ms = self.kernel_ms
        both.series = np.concatenate([self.series, other.series])
        both._active = list(range(len(rows)))
        both._lazy = (both.series, both._active)
        both._detect_locks()
        return both

    def showTrackingQuality(self):
        """ASCII table of .quality, in the manner of AcquisitionResult.showChannelStatus."""
        q = self.quality
        bar = '*=========*=====*=============*===============*============*'
        print('\n' + bar)
        print('| Channel | PRN | C/N0 dB-Hz  | carrier lock  |  Lost at   |')
        print(bar)
        for j, r in enumerate(q):
            lock = np.asarray(r.carrLock, dtype=np.float64)
            if r.lostAtMs >= 0:                                   # the windows before the loss, as for medianCNo
                lock = lock[:r.lostAtMs // int(round(float(self._settings.cnoInterval))) - 1]
            lock = lock[np.isfinite(lock)]
            print('|      %2d | %3d |   %7.2f   |    %6.3f     | %s |' % (
                j, int(r.PRN), r.medianCNo, float(np.median(lock)) if lock.size else np.nan,
                ('%7d ms' % r.lostAtMs) if r.lostAtMs >= 0 else '      --  '))
        print(bar + '\n')

    def _detect_locks(self):
        """lockDetector: the quality right after tracking, and status '-' for every channel it declares lost."""
        if getattr(self._settings, "lockDetector", False) and self.has_results():
            self._lost_rows = tuple(int(j) for j in np.flatnonzero(self.quality.lostAtMs >= 0))

    def _data_type(self):
        """Settings.dataType -> (sgx_track_ex data_type, bytes per sample).  The reference reads np.fromfile(fid,
        dataType, blksize) (tracking.py:154) but seeks and tells in BYTES (tracking.py:107, 255): both are kept."""
        dt = np.dtype(self._settings.dataType)
        key = dt.kind + str(dt.itemsize)
        # int8 / uint8 / int16 have their own kernels; float32 records of integers times one power of two are narrowed
        # to them exactly; every other real type is read sample by sample where it lies (include/sgx.h, sgx_track_ex)
        little = dt.byteorder in ('<', '|') or (dt.byteorder == '=' and np.little_endian)
        if key in _DT_CODES and little:
            return _DT_CODES[key], dt.itemsize
        raise TypeError("the GPU path tracks little-endian real IF samples - int8 ... uint64, float16 / 32 / 64 - not "
                        "Settings.dataType %r" % (self._settings.dataType,))

    def _window(self, fid, first, need):
        """Bytes [first, first+need) of the reference's file, as an HBM record."""
        ctx = engine.get_context(self._settings, self._device)
        dtype_code, isz = self._data_type()
        # a real file on disk: stream it natively (pinned double buffering, no numpy copy of the record), and let
        # tracking start while the transfer is still running
        name = getattr(fid, 'name', None)
        if isinstance(name, (str, bytes)) and os.path.isfile(name):
            return ctx.open_file(name, first, need)      # fills in the background; the kernel follows the watermark
        fid.seek(first, 0)
        if hasattr(fid, 'fileno'):
            try:
                data = np.fromfile(fid, np.int8, need)
            except (OSError, ValueError, AttributeError):
                data = np.frombuffer(fid.read(need), dtype=np.int8)
        else:
            data = np.frombuffer(fid.read(need), dtype=np.int8)
        return ctx.upload(data)

    @contextlib.contextmanager
    def _record(self, fid, first, need):
        """(the record a launch runs on, the file offset of its first byte): a DeviceFile's resident record, or bytes
        [first, first + need()) of the reference's file in a record of this call's own, freed on the way out."""
        if isinstance(fid, DeviceFile):
            yield fid.record, fid.file_offset
            return
        # the window starts on a 4 KiB boundary of the FILE: page-aligned reads, and every sample keeps the place
        # inside its 16-byte group that it has in a record resident from file offset 0 - the kernel's lanes then
        # add the same samples in the same order, and the series are bit-identical to the resident run's
        start = (first // 4096) * 4096
        rec = self._window(fid, start, first - start + need())
        try:
            yield rec, start
        finally:
            rec.free()

    def _finish(self, fid, series, active, done, ms):
        """The tail of a launch, eager or chained.  series: float64[len(active), 13, ms], done: ms completed per row."""
        if not active:
            self._results = np.recarray((0,), dtype=RESULT_DTYPE)
            self.series = np.empty((0, _native.NUM_SERIES, ms))
            return
        if np.any(done != ms):
            print('Not able to read the specified number of samples for tracking, exiting!')
            fid.close()
            return
        if self._verbose:
            channel, nch = self._channels, int(self._settings.numberOfChannels)
            for i in active:
                for k in range(0, ms, 50):
                    print('Tracking: Ch %d' % (i + 1) + ' of %d' % nch + '; PRN#%02d' % int(channel[i].PRN) +
                          '; Completed %d' % k + ' of %d' % ms + ' msec')
        fid.seek(int(series[-1, 0, ms - 1]), 0)    # where the reference's last read left the file
        self.series = series
        self._lazy = (series, active)              # the record array of object fields is packed on first access of .results
        self._active = active
        self._detect_locks()

    def track(self, fid):
        """Code and carrier tracking of all channels (reference tracking.py:13-295).

        fid   open binary file of Settings.dataType samples (any real little-endian type; seek/read/tell/close), or a
              DeviceFile over a record already in HBM (for int16: the file's bytes, Context.upload_bytes).  Each active channel starts at byte
              skipNumberOfBytes + codePhase (tracking.py:107).
        On a short record the reference prints a message, closes fid and returns None without
        setting results (tracking.py:159-163); so does this method.
        """
        settings = self._settings
        ctx = engine.get_context(settings, self._device)
        ms = int(settings.msToProcess)            # float in the reference (Q9)
        nch = int(settings.numberOfChannels)
        self._reset()
        coherent = int(getattr(settings, "trackCoherentMs", 1))
        if coherent > 1:
            return self._track_coherent(fid, ctx, nch, ms)
        if self._channels is None and self._try_chained(fid, ctx, nch, ms):
            return
        channel = self._table()   # (where the queued sequence did not apply: the search is looked at, preRun runs here)
        active = [i for i in range(nch) if channel[i].PRN != 0]
        if not active:
            return self._finish(fid, None, active, None, ms)
        chans = [(int(channel[i].PRN), float(channel[i].acquiredFreq), float(channel[i].codePhase))
                 for i in active]
        dtype_code, isz = self._data_type()
        first = int(settings.skipNumberOfBytes + min(c[2] for c in chans))
        last = int(settings.skipNumberOfBytes + max(c[2] for c in chans))

        def need():
            n = settings.samplesPerCode
            return last - first + (ms * (n + 2) + n) * isz   # a block is at most samplesPerCode + 1 long
        with self._record(fid, first, need) as (rec, file_off):
            series, done = ctx.track(rec, chans, ms, rec_file_offset=file_off, data_type=dtype_code)
            self.kernel_ms = ctx.timing()["track_ms"]
        self._finish(fid, series, active, done, ms)

    def _track_coherent(self, fid, ctx, nch, ms):
        """Settings.trackCoherentMs > 1: the record as track() loads it, every channel through sgx_track_coherent (the
        bit edges found during the pull-in), .series / .results as ever - the six sums, absoluteSample and the rates are
        per block - plus .bitEdge, .coherentStart (int32 per row) and .edgeEnergy (float64[n, 20])."""
        settings = self._settings
        dtype_code, isz = self._data_type()
        if dtype_code != _native.DT_INT8:
            raise TypeError("coherent tracking (trackCoherentMs %d) reads int8 records, not Settings.dataType %r: the "
                            "conditioning and requantising stages make one" % (int(settings.trackCoherentMs), settings.dataType))
        channel = self._table()
        active = [i for i in range(nch) if channel[i].PRN != 0]
        if not active:
            return self._finish(fid, None, active, None, ms)
        chans = [(int(channel[i].PRN), float(channel[i].acquiredFreq), float(channel[i].codePhase)) for i in active]
        first = int(settings.skipNumberOfBytes + min(c[2] for c in chans))
        last = int(settings.skipNumberOfBytes + max(c[2] for c in chans))

        def need():
            n = settings.samplesPerCode
            return last - first + ms * (n + 2) + n
        params = _native.coh_params(settings)
        with self._record(fid, first, need) as (rec, file_off):
            rec.wait()          # (a record still streaming in: the kernel follows no watermark)
            series, done, edge, start, energy = ctx.track_coherent(rec, chans, ms, params, rec_file_offset=file_off)
            self.kernel_ms = ctx.timing()["track_ms"]
        self._finish(fid, series, active, done, ms)
        if self.series is not None:
            self.bitEdge, self.coherentStart, self.edgeEnergy = edge, start, energy

    def _try_chained(self, fid, ctx, nch, ms):
        """The record is resident, and the acquisition's search and its preRun are still queued on this context: preRun
        runs on the device, the tracking kernel behind it, and the host waits once (AcquisitionResult.track_chained).
        False: not applicable - the eager sequence follows."""
        if not (isinstance(fid, DeviceFile) and not self._verbose and 1 <= nch <= 32):
            return False
        try:
            dtype_code, isz = self._data_type()
        except TypeError:
            return False
        got = self._acq.track_chained(ctx, fid.record, nch, ms, rec_file_offset=fid.file_offset, data_type=dtype_code)
        if got is None:
            return False
        out, done, n_act, self._channels = got           # (the table: what preRun made, on the device)
        self.chained = True
        self.kernel_ms = ctx.timing()["track_ms"]
        self._finish(fid, out[:n_act], list(range(n_act)), done[:n_act], ms)
        return True

    def plot(self):
        """One figure per tracked channel: discrete-time scatter, navigation bits, raw and filtered discriminators,
        correlator magnitudes (the panels of reference tracking.py:297-426).  Needs matplotlib; prints a notice
        and returns without it."""
        from .initialize import _pyplot
        plt = _pyplot("TrackingResult.plot")
        if plt is None:
            return
        assert isinstance(self._results, np.recarray)
        t = np.arange(int(self._settings.msToProcess)) / 1000.0
        for k, r in enumerate(self._results):
            plt.figure(200 + k)
            plt.clf()
            plt.suptitle('Channel %d (PRN %d) results' % (k, int(r.PRN)))
            ax = plt.subplot(3, 3, 1)
            ax.plot(r.I_P, r.Q_P, '.')
            ax.set_title('Discrete-Time Scatter Plot')
            ax.set_xlabel('I prompt')
            ax.set_ylabel('Q prompt')
            ax.axis('equal')
            ax = plt.subplot(3, 3, (2, 3))
            ax.plot(t, r.I_P)
            ax.set_title('Bits of the navigation message')
            ax.set_xlabel('Time (s)')
            for pos, series, title in ((4, r.pllDiscr, 'Raw PLL discriminator'), (7, r.pllDiscrFilt, 'Filtered PLL discriminator'),
                                       (6, r.dllDiscr, 'Raw DLL discriminator'), (9, r.dllDiscrFilt, 'Filtered DLL discriminator')):
                ax = plt.subplot(3, 3, pos)
                ax.plot(t, series)
                ax.set_title(title)
                ax.set_xlabel('Time (s)')
            ax = plt.subplot(3, 3, (5, 8))
            ax.plot(t, np.sqrt(r.I_E ** 2 + r.Q_E ** 2), t, np.sqrt(r.I_P ** 2 + r.Q_P ** 2),
                    t, np.sqrt(r.I_L ** 2 + r.Q_L ** 2), '-*')
            ax.set_title('Correlation results')
            ax.set_xlabel('Time (s)')
            ax.legend(['E', 'P', 'L'])
