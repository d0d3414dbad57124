"""Settings / Result / TruePosition with the reference's names (reference initialize.py:20-185).

The three helpers the hot path calls - generateCAcode, makeCaTable, calcLoopCoef - are answered
by libsgx.so's exact host routines (include/sgx.h), not by Python arithmetic.
"""
import contextlib
import copy
import ctypes as C
import datetime
import os

import numpy as np

from . import _native


class Result(object):
    """Base of AcquisitionResult / TrackingResult (reference initialize.py:20-46)."""

    def __init__(self, settings):
        self._settings = settings
        self._results = None
        self._channels = None
        self._merged = None

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
        self._merged = None        # (AcquisitionResult: arrays of a sharded search not yet packed)
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

# narrowband interference excision ahead of acquisition (Settings.mitigate; INTEGRATION.md, "Interference excision"):
# continuous-wave lines found in the Welch spectrum of probeData are notched out of the record by a zero-phase integer FIR
_NOTCH_DEFAULTS = (
    ("interferenceMitigation", False),   # postProcessing() filters the record before acquisition and tracking
    ("notchThresholdDb", 8.0),           # a PSD bin this far above the running median of its neighbourhood is a line
    ("notchWidthHz", 80e3),              # least width of a notch
    ("notchTaps", 1025),                 # filter length (odd, at most 4095)
)

# interleaved 8-bit I/Q baseband records (Settings.convertIQ; INTEGRATION.md, "I/Q baseband records"): the file is turned
# into the equivalent real IF record on the GPU and every stage runs on that, under Settings.realEquivalent()
_IQ_DEFAULTS = (
    ("iqRecord", False),                 # fileName holds interleaved I/Q: samplingFreq is the COMPLEX rate, IF the baseband
                                         # offset (0 or negative allowed), dataType 'int8' or 'uint8' (offset binary)
    ("iqQFirst", False),                 # the file holds Q before I (also: spectral inversion of an I-first file)
    ("iqTaps", 63),                      # length of the interpolation filter (odd, at most 255)
    # int16 (sc16) and float32 (fc32) I/Q files (Settings.requantizeIQ; INTEGRATION.md, "int16 / float32 I/Q"): the file is
    # brought to int8 on the GPU through one fixed gain, ahead of the converter
    ("iqRequantize", False),             # with iqRecord: dataType 'int16' and 'float32' are read through the requantiser
    ("iqTargetRms", 12.0),               # rms of the int8 record it makes, LSB, in (0, 127]
)

# block-wise front-end conditioning (Settings.conditionRecord; INTEGRATION.md, "Front-end conditioning"): DC removal, a
# time-varying AGC and pulse blanking per short block, first of all stages, where the fixed-gain requantiser sits otherwise
_COND_DEFAULTS = (
    ("frontEndConditioning", False),     # the stage is off
    ("condBlockUs", 100.0),              # block length: that many frames at samplingFreq, to a multiple of 16 in 256 .. 16384
    ("condAgcBlocks", 32.0),             # the AGC's smoothing length in blocks
    ("condBlankFactor", 4.0),            # c: a frame beyond c x the smoothed rms is blanked; blank_q4 = rint(16 c^2); 0: off
    ("condGuardFrames", 8),              # frames blanked either side of a hit
    ("condTargetRms", 12.0),             # rms of the int8 record it makes, LSB, in (0, 127]
)

# 1-, 2- and 4-bit packed records (Settings.unpackRecord; INTEGRATION.md, "Packed records"): the file is unpacked to one int8
# sample per selected field on the GPU, first of all stages
_PACK_DEFAULTS = (
    ("packedBits", 0),                   # bits per sample of the file: 1, 2 or 4; 0: the stage is off
    ("packedEncoding", 'sign-magnitude'),   # or 'offset-binary', 'twos-complement': what a code means
    ("packedLsbFirst", False),           # the first sample of a byte lies in its low bits
    ("packedFrame", 1),                  # F: fields per frame (1, 2, 4, 8 or 16) of a file that interleaves several streams
    ("packedFirst", 0),                  # the field of a frame the selection starts at
    ("packedPeak", 48),                  # the largest level of the int8 record it makes, LSB, in 2^bits - 1 .. 127
    ("packedTable", None),               # an explicit sequence of 2^bits int8 levels, one per code: overrides encoding and peak
)

# band selection and decimation ahead of acquisition (Settings.decimateRecord; INTEGRATION.md, "Decimation"): the int8 record
# goes through a band-pass around the carrier and comes out at 1 / decimation of the rate, behind the unpacker, the
# conditioning stage and the requantiser, in front of the I/Q converter and the notch
_DECIM_DEFAULTS = (
    ("decimation", 0),                   # the factor D, 2 .. 16; 0: the stage is off
    ("decimTaps", 127),                  # filter length (odd, at most 511)
    ("decimBandwidth", 2.046e6),         # two-sided bandwidth of the band that is kept, Hz
    ("decimGain", 0.0),                  # 0: the gain that keeps a white input's rms
)

# rational resampling ahead of acquisition (Settings.resampleRecord; INTEGRATION.md, "Resampling"): the real int8 record goes
# through a polyphase low-pass and comes out at resampleUp / resampleDown of the rate, behind the unpacker, the conditioning
# stage or requantiser, the decimator and the I/Q converter, in front of the notch - a capture below the 15.4 samples per
# chip the fast tracking kernels need reaches them
_RESAMP_DEFAULTS = (
    ("resampleUp", 0),                   # the up factor L, 2 .. 16; 0: the stage is off
    ("resampleDown", 1),                 # the down factor M, 1 .. 3, below L and coprime to it
    ("resampTaps", 0),                   # filter length at the stuffed rate (odd, at most 1023); 0: 24 L + 1
    ("resampCutoff", 0.0),               # cutoff of the low-pass, Hz; 0: half the lower of the two rates
    ("resampGain", 1.0),
)


class Settings(object):
    """Receiver configuration; attribute names and defaults of reference initialize.py:81-173."""

    c = property(lambda self: 299792458.0, doc="speed of light, m/s (read-only, initialize.py:170)")
    startOffset = property(lambda self: 68.802, doc="initial travel-time guess, ms (read-only, initialize.py:172)")

    def __init__(self):
        for name, value in _DEFAULTS + _LOCK_DEFAULTS + _ACQ_DEFAULTS + _NOTCH_DEFAULTS + _IQ_DEFAULTS + _COND_DEFAULTS \
                + _PACK_DEFAULTS + _DECIM_DEFAULTS + _RESAMP_DEFAULTS:
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

    def mitigate(self, record, offset=0, device=None):
        """Narrowband interference excision of a resident int8 record (a _native.Record): the Welch spectrum of the 10 code
        periods from sample `offset` (probe_stats, as probeData), its lines by notchThresholdDb / notchWidthHz, a notch of
        notchTaps taps (notch_design) and, if there is a line, the whole record through it (filter_record).  Returns
        (record, lines): a NEW record of the same length - sample n lines up with sample n of the old one - or the SAME
        record when no line was found; lines is a list of (centre Hz, width Hz).  The caller frees what it gets."""
        from . import engine
        if np.dtype(self.dataType) != np.dtype(np.int8):
            raise ValueError("interference excision filters int8 records only, not Settings.dataType %r" % (self.dataType,))
        ctx = record.ctx if device is None else engine.get_context(self, device)
        n = min(10 * self.samplesPerCode, len(record) - int(offset))
        f, pxx, _, _ = ctx.probe_stats(record, int(offset), n, self.samplingFreq / 1000000.0)
        taps, shift, lines = _native.notch_design(self, f, pxx, self.notchThresholdDb, self.notchWidthHz, self.notchTaps)
        if not lines:
            return record, lines
        return ctx.filter_record(record, taps, shift), lines

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

    def _iq_width(self):
        """Bytes per component of the I/Q file: 2 or 4 where it goes through the requantiser or the conditioning stage,
        else 1."""
        self._iq_format()
        return np.dtype(self.dataType).itemsize if self.iqRecord else 1

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

    def _pack_format(self):
        """(bits, lsb_first, frame, first, take, table) of the unpacker for these settings.  take: a frame of several
        fields (packedFrame > 1) gives its I/Q pair with iqRecord, else one field; with packedFrame = 1 every field is
        taken (I and Q simply alternate, the converter sorts them out)."""
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

    def _unpacked_settings(self):
        """The settings the UNPACKED record is read under: a copy with the stage off, int8, and skipNumberOfBytes turned
        from a byte of the packed file (on a frame boundary) into the sample it becomes, skip 8 take / (b F)."""
        unit, samples = self._pack_units()
        skip = int(self.skipNumberOfBytes)
        if skip % unit:
            raise ValueError("skipNumberOfBytes = %d splits a frame of the packed file: it must be a multiple of %d"
                             % (skip, unit))
        un = copy.copy(self)
        un.packedBits = 0
        un.skipNumberOfBytes = skip // unit * samples
        return un

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

    def _prepared_settings(self):
        """The settings the PREPARED record is read under: realEquivalent(), with skipNumberOfBytes turned from a byte of a
        file of w-byte components into the sample of the prepared record it becomes, skipNumberOfBytes / w.  A real record
        that goes through the conditioning stage comes out as int8 in the same way; a packed record (packedBits) is read
        as the int8 record the unpacker makes of it (_unpacked_settings), whatever follows; a record that is decimated
        (decimation) as the int8 record the decimator makes of it (_decimated_settings), whatever follows that; a record
        that is resampled (resampleUp) as the record the resampler makes of all that (_resampled_settings)."""
        if self.resampleUp:
            return self._resampled_settings()
        if self.packedBits:
            return self._unpacked_settings()._prepared_settings()
        if self.decimation:
            return self._decimated_settings()._prepared_settings()
        if not self.iqRecord:
            if not self.frontEndConditioning:
                return self
            w = self._cond_format()[0]
            real = copy.copy(self)
            real.frontEndConditioning = False
            real.dataType = 'int8'
            skip = int(self.skipNumberOfBytes)
            if skip % w:
                raise ValueError("skipNumberOfBytes = %d splits a sample: it must be a multiple of %d" % (skip, w))
            real.skipNumberOfBytes = skip // w
            return real
        real = self.realEquivalent()
        real.frontEndConditioning = False            # (the prepared record has been through the stage)
        w = self._iq_width()
        skip = int(self.skipNumberOfBytes)
        if skip % (2 * w):
            raise ValueError("skipNumberOfBytes = %d splits an I/Q pair: it must be %s" %
                             (skip, "even" if w == 1 else "a multiple of %d (pairs of %d-byte components)" % (2 * w, w)))
        real.skipNumberOfBytes = skip // w
        return real

    def _resamp_front(self):
        """The settings of the record the resampler READS: the prepared settings of a copy with the stage off."""
        off = copy.copy(self)
        off.resampleUp = 0
        front = off._prepared_settings()
        if np.dtype(front.dataType) != np.dtype(np.int8):
            raise ValueError("Settings.resampleUp reads a real record as int8: Settings.dataType %r is resampled only behind a "
                             "stage that makes int8 of it (Settings.frontEndConditioning, Settings.packedBits, "
                             "Settings.iqRecord)" % (self.dataType,))
        return front

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
        record the stage reads; info: fs_out, cutoff).  The C/A band of that record, up to IF + 1.023 MHz, must lie below
        the cutoff."""
        L, M, Lh = self._resamp_format()
        front = self._resamp_front()
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

    def _resampled_settings(self):
        """The settings the RESAMPLED record is read under: those of the record the stage reads (_resamp_front), with
        samplingFreq L / M, the IF unchanged, and skipNumberOfBytes - there a sample, on a multiple of M - turned into the
        sample of the resampled record it becomes, skip L / M."""
        L, M, _ = self._resamp_format()
        front = self._resamp_front()
        _, _, info = self._resamp_design()
        skip = int(front.skipNumberOfBytes)
        if skip % M:
            raise ValueError("skipNumberOfBytes = %d: sample %d of the record the resampler reads does not map to a whole "
                             "sample at %d / %d of the rate: it must be a multiple of Settings.resampleDown = %d"
                             % (int(self.skipNumberOfBytes), skip, L, M, M))
        res = copy.copy(front)
        res.samplingFreq = info["fs_out"]
        res.skipNumberOfBytes = skip // M * L
        return res

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

    def _decimated_settings(self):
        """The settings the DECIMATED record is read under: a copy with the stage off, int8 (conditioned and requantised
        where the settings say so), samplingFreq / decimation, the IF where the band lands (info f_out of _decim_design)
        and skipNumberOfBytes turned from a byte of a file of w-byte components - on a multiple of `decimation` frames -
        into the byte of the decimated record it becomes."""
        lanes, D, _, _, _ = self._decim_format()
        _, _, info = self._decim_design()
        if self.iqRecord:
            w = self._iq_width()
        else:
            w = self._cond_format()[0] if self.frontEndConditioning else 1
        skip = int(self.skipNumberOfBytes)
        if skip % (w * lanes * D):
            raise ValueError("skipNumberOfBytes = %d does not fall on a multiple of Settings.decimation = %d %s: it must be a "
                             "multiple of %d" % (skip, D, "I/Q pairs" if lanes == 2 else "samples", w * lanes * D))
        dec = copy.copy(self)
        dec.decimation = 0
        dec.frontEndConditioning = False
        dec.iqRequantize = False
        dec.dataType = 'int8'
        dec.samplingFreq = info["fs_out"]
        dec.IF = info["f_out"]
        dec.skipNumberOfBytes = skip // (w * D)
        return dec

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

    def realEquivalent(self):
        """The settings of the real IF record that convertIQ makes of the I/Q file these settings describe: a copy with
        samplingFreq * 2, IF + samplingFreq / 2, iqRecord = False and dataType 'int8' (what the converter writes).
        Without iqRecord the record is real already: a plain copy."""
        real = copy.copy(self)
        if self.iqRecord:
            real.samplingFreq = 2.0 * self.samplingFreq
            real.IF = self.IF + self.samplingFreq / 2.0
            real.iqRecord = False
            real.dataType = 'int8'
        return real

    def convertIQ(self, record):
        """A resident record holding the raw bytes of an interleaved 8-bit I/Q file (a _native.Record) as the equivalent
        real IF record (iq_to_if through the iqTaps-tap filter of iq_design): a NEW int8 record of the same length whose
        sample n is the instant of byte n's pair, to be read under realEquivalent().  The caller frees both."""
        q_first, offset_binary = self._iq_format()
        taps, shift = _native.iq_design(self.iqTaps)
        return record.ctx.iq_to_if(record, taps, shift, q_first=q_first, offset_binary=offset_binary)

    @contextlib.contextmanager
    def _prepared_record(self, name, offset, count, mitigate_at=None, verbose=False):
        """Samples [offset, offset + count) of the prepared record of a record file, uploaded once and prepared on the
        GPU, for the length of the block: with packedBits unpacked to int8 (unpackRecord), first of all - offset must then
        fall on a frame boundary of the file, and count is rounded up to whole frames; with
        frontEndConditioning brought to int8 block by block (conditionRecord), first
        of all; with iqRequantize and an int16 / float32 dataType brought to int8 (requantizeIQ),
        with decimation brought to 1 / decimation of the rate (decimateRecord), with iqRecord converted to real IF (the sample
        of the converter's record that offset stands for must then be even, the first byte of a pair), with
        resampleUp = L brought to L / M of the rate (resampleRecord; offset must then be a multiple of L: sample offset of
        the prepared record is sample offset M / L of the record the stage reads), with
        mitigate_at (a sample of the prepared record; None: no mitigation) cleared
        of the narrowband lines in the spectrum from there on - the conversion first, the notch is designed at the real
        rate.  offset and count are in BYTES OF THE PREPARED RECORD: for a file of w-byte components the bytes
        [w offset, w (offset + count)) are read, and sample n of the prepared record is file byte n w; with decimation = D
        the bytes [w D offset, w D (offset + count)), whole groups of D frames.  Each intermediate
        record is freed as soon as the next one exists.  Yields the prepared record, to be read under
        _prepared_settings(), and frees it afterwards."""
        from . import engine
        say = print if verbose else (lambda *args: None)
        real = self._prepared_settings()
        w = self._iq_width() if self.iqRecord else (self._cond_format()[0] if self.frontEndConditioning else 1)
        front = self                                 # the settings the converter reads its input under
        if self.resampleUp:
            # sample n L of the prepared record is sample n M of the record the resampler reads
            L, M, _ = self._resamp_format()
            if offset % L:
                raise ValueError("sample %d of the resampled record is not a sample of the record the resampler reads: it "
                                 "must be a multiple of Settings.resampleUp = %d" % (offset, L))
            offset, count = offset // L * M, -(-count * M // L)
            if self.iqRecord:
                count += count % 2                   # (whole pairs)
        if self.iqRecord and offset % 2:
            # byte n of the converted record is the instant of byte n's pair; ahead of the decimator's * D, behind which an
            # odd sample of an even D would pass as a pair - and the upload would start on a Q, read as I from there on
            raise ValueError("sample %d of the record the I/Q converter makes splits an I/Q pair of the record it reads: it "
                             "must be even" % offset)
        if self.decimation:
            # sample n of the prepared record is sample n D of the record the decimator reads
            front = (self._unpacked_settings() if self.packedBits else self)._decimated_settings()
            offset, count = offset * int(self.decimation), count * int(self.decimation)
        if self.packedBits:
            unit, samples = self._pack_units()
            if offset % samples:
                raise ValueError("sample %d of the unpacked record does not start a frame of the packed file: it must be a "
                                 "multiple of %d" % (offset, samples))
            units = -(-count // samples)                                  # (with iqRecord `samples` is even: whole pairs)
            file_off = offset // samples * unit
            whole = max(0, os.path.getsize(name) - file_off) // unit      # (a file that ends inside a frame: the frame is left)
            rec = engine.get_context(real, None).upload_file(name, file_off, min(units, whole) * unit)
        else:
            rec = engine.get_context(real, None).upload_file(name, w * offset, w * count)
        try:
            if self.packedBits:
                say('   Unpacking %d-bit samples to int8...' % int(self.packedBits))
                raw, rec = rec, None
                try:
                    rec, info = self.unpackRecord(raw)
                finally:
                    raw.free()
                say('   %d samples; levels %s' % (info["samples"], ", ".join(
                    "%+d: %.2f %%" % (int(lv), 100.0 * sh) for lv, sh in sorted(zip(info["table"], info["shares"])))))
            if self.frontEndConditioning:
                say('   Conditioning %s samples block by block...' % np.dtype(self.dataType).name)
                raw, rec = rec, None
                try:
                    rec, info = self.conditionRecord(raw)
                finally:
                    raw.free()
                say('   %d blocks of %d frames: gain %+.2f .. %+.2f dB, %.4f %% of the frames blanked, %.4f %% of the '
                    'samples clipped' % (info["blocks"], info["block"], info["gain_db_min"], info["gain_db_max"],
                                         100.0 * info["blanked"], 100.0 * info["clipped"]))
            elif w > 1:
                say('   Requantising %s samples to int8...' % np.dtype(self.dataType).name)
                raw, rec = rec, None
                try:
                    rec, info = self.requantizeIQ(raw)
                finally:
                    raw.free()
                say('   rms %.6g, peak %.6g, %d non-finite samples, gain %+.2f dB, %.4f %% of the samples clipped'
                    % (info["rms"], info["max_abs"], info["n_nonfinite"], info["gain_db"], 100.0 * info["clipped"]))
            if self.decimation:
                say('   Decimating by %d through %d taps...' % (int(self.decimation), int(self.decimTaps)))
                raw, rec = rec, None
                try:
                    rec, info = self.decimateRecord(raw)
                finally:
                    raw.free()
                say('   %d samples at %.6g Msps, %s %.6g MHz, band %s, %.4f %% of the samples clipped'
                    % (info["samples"], info["fs_out"] / 1e6, "carrier at" if self.iqRecord else "IF", info["f_out"] / 1e6,
                       "INVERTED (Doppler shows with the other sign)" if info["inverted"] else "upright",
                       100.0 * info["clipped"]))
            if self.iqRecord:
                say('   Converting I/Q at %.6g Msps to real IF: %.6g Msps, IF %.6g MHz...'
                    % (front.samplingFreq / 1e6, real.samplingFreq / 1e6, real.IF / 1e6))
                raw, rec = rec, None
                try:
                    rec = front.convertIQ(raw)
                finally:
                    raw.free()
            if self.resampleUp:
                L, M, Lh = self._resamp_format()
                say('   Resampling by %d/%d through %d taps...' % (L, M, Lh))
                raw, rec = rec, None
                try:
                    rec, info = self.resampleRecord(raw)
                finally:
                    raw.free()
                say('   %d samples at %.6g Msps, %.4f %% of the samples clipped'
                    % (info["samples"], info["fs_out"] / 1e6, 100.0 * info["clipped"]))
            if mitigate_at is not None:
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
            yield rec
        finally:
            if rec is not None:
                rec.free()

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
        return acqResults, trackResults

    def _resident_processing(self, name):
        """postProcessing()'s acquire -> preRun -> track on a record that _prepared_record uploads once and prepares on the
        GPU; both stages read the prepared record where it lies.  The results carry _prepared_settings(): positions
        (codePhase, absoluteSample, skipNumberOfBytes) are samples of the prepared record, which are bytes of an 8-bit file
        and file byte / w of a file of w-byte components (int16: w = 2, float32: w = 4, with iqRequantize); of a packed
        file (packedBits = b, frames of F fields of which `take` are kept) sample n is byte n b F / (8 take).  With
        decimation = D a sample of the prepared record is D samples of the record in front of the stage (I/Q: D pairs),
        so the upload holds whole groups of D frames."""
        from .record import DeviceFile, DeviceSignal
        real = self._prepared_settings()
        n = real.samplesPerCode
        skip = int(real.skipNumberOfBytes)
        need = skip + max(real.acquisitionLength(), int(self.msToProcess) * (n + 2) + 2 * n)
        if self.iqRecord:
            need += need % 2                         # (whole pairs; with decimation: whole groups of D pairs)
        with self._prepared_record(name, 0, need, skip if self.interferenceMitigation else None, verbose=True) as rec:
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
        if self.iqRecord or self.interferenceMitigation or self.frontEndConditioning or self.packedBits or self.decimation \
                or self.resampleUp:
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
