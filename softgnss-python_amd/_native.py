"""ctypes binding of libsgx.so (include/sgx.h).  No torch, no fallback.

The product path fails loudly: if the library is missing, or a device entry point is called
without a GPU, an exception is raised - there is no CPU implementation behind these calls.
"""
import ctypes as C
import os
import threading
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SGX_LIB") or os.path.join(HERE, "lib", "libsgx.so")   # SGX_LIB: another build of the same library (kernel variants side by side)

SGX_OK = 0
SGX_E_ARG, SGX_E_HIP, SGX_E_NOMEM, SGX_E_INDEX, SGX_E_RCCL, SGX_E_RANGE, SGX_E_DEFER = -1, -2, -3, -4, -5, -6, -7
SGX_E_SILENT = -8
NUM_SERIES = 13
DT_INT8, DT_INT16, DT_UINT8, DT_FLOAT32 = 0, 1, 2, 3   # sgx_track_ex data_type (include/sgx.h)
DT_FLOAT64, DT_UINT16, DT_INT32, DT_UINT32, DT_INT64, DT_UINT64, DT_FLOAT16 = 4, 5, 6, 7, 8, 9, 10
MAX_SATS = 16
SERIES = ("absoluteSample", "codeFreq", "carrFreq", "I_P", "I_E", "I_L", "Q_E", "Q_P", "Q_L",
          "dllDiscr", "dllDiscrFilt", "pllDiscr", "pllDiscrFilt")


class SgxError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "libsgx error %d: %s" % (code, msg))
        self.code = code


class SilentChannelError(ValueError):
    """The reference's ValueError on a channel that went silent (SGX_E_SILENT: a block of exactly zero sums leaves the
    rates NaN, and int(np.ceil(nan)) of the next block's length raises, tracking.py:148-151).  Where the call had
    results to return they are attached: .series float64[n_ch, 13, ms] and .ms_done int32[n_ch], complete as after a
    call that returned (the silent block is the channel's last row, the rows behind it hold the pre-fill)."""

    def __init__(self, msg, series=None, ms_done=None):
        ValueError.__init__(self, msg)
        self.code = SGX_E_SILENT
        self.series, self.ms_done = series, ms_done


class Settings(C.Structure):
    _fields_ = [("samplingFreq", C.c_double), ("IF", C.c_double), ("codeFreqBasis", C.c_double),
                ("acqSearchBand", C.c_double), ("acqThreshold", C.c_double),
                ("dllDampingRatio", C.c_double), ("dllNoiseBandwidth", C.c_double),
                ("dllCorrelatorSpacing", C.c_double), ("pllDampingRatio", C.c_double),
                ("pllNoiseBandwidth", C.c_double), ("skipNumberOfBytes", C.c_int64),
                ("codeLength", C.c_int32), ("numberOfChannels", C.c_int32)]


class ChanInit(C.Structure):
    _fields_ = [("acquiredFreq", C.c_double), ("codePhase", C.c_double), ("prn", C.c_int32),
                ("reserved", C.c_int32)]


class Sat(C.Structure):
    _fields_ = [("code_fcw", C.c_uint64), ("code_c0", C.c_uint64), ("nav_seed", C.c_uint64),
                ("car_fcw", C.c_uint32), ("car_ph0", C.c_uint32), ("prn", C.c_int32), ("amp", C.c_int32)]


class Scene(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("n_sats", C.c_int32), ("nav_mode", C.c_int32),
                ("sats", Sat * MAX_SATS), ("cos_lut", C.c_int16 * 256), ("nav_bits", (C.c_uint8 * 256) * MAX_SATS)]


class Timing(C.Structure):
    _fields_ = [("acquire_ms", C.c_float), ("acq_coarse_ms", C.c_float), ("acq_fine_ms", C.c_float),
                ("track_ms", C.c_float), ("synth_ms", C.c_float), ("track_kernel", C.c_float),
                ("track_members", C.c_float), ("track_streamed", C.c_float)]


class AcqParams(C.Structure):
    """sgx_acq_params: a coherent multi-millisecond search (sgx_acquire_coherent, 24 bytes)."""
    _fields_ = [("coherent_ms", C.c_int32), ("n_windows", C.c_int32), ("noncoh", C.c_int32), ("reserved", C.c_int32),
                ("bin_step_hz", C.c_double)]


def acq_params(coherent_ms=1, n_windows=2, noncoh=False, bin_step_hz=None):
    """AcqParams with the default step 500 / coherent_ms Hz where bin_step_hz is None."""
    step = 500.0 / int(coherent_ms) if bin_step_hz is None and int(coherent_ms) > 0 else bin_step_hz
    return AcqParams(int(coherent_ms), int(n_windows), 1 if noncoh else 0, 0, float(step if step is not None else 0.0))


class CohParams(C.Structure):
    """sgx_coh_params: the coherent loops and the schedule of sgx_track_coherent (64 bytes)."""
    _fields_ = [("tau1_pll", C.c_double), ("tau2_pll", C.c_double), ("tau1_dll", C.c_double), ("tau2_dll", C.c_double),
                ("coherent_ms", C.c_int32), ("pull_in_ms", C.c_int32), ("handover_ms", C.c_int32), ("reserved", C.c_int32),
                ("reserved2", C.c_double * 2)]


def coh_params(settings, coherent_ms=None, pull_in_ms=None, handover_ms=None):
    """CohParams of a Settings-like object: trackCoherentMs, trackPullInMs, trackHandOverMs (or the arguments), and the
    coherent loops' coefficients from cohPllNoiseBandwidth / cohDllNoiseBandwidth with the settings' damping ratios."""
    t1p, t2p, t1d, t2d = C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0)
    check(lib().sgx_calc_loop_coef(float(getattr(settings, "cohPllNoiseBandwidth", 3.0)), float(settings.pllDampingRatio),
                                   0.25, C.byref(t1p), C.byref(t2p)))
    check(lib().sgx_calc_loop_coef(float(getattr(settings, "cohDllNoiseBandwidth", 1.0)), float(settings.dllDampingRatio),
                                   1.0, C.byref(t1d), C.byref(t2d)))
    pick = lambda given, name, default: int(getattr(settings, name, default) if given is None else given)
    return CohParams(t1p.value, t2p.value, t1d.value, t2d.value, pick(coherent_ms, "trackCoherentMs", 1),
                     pick(pull_in_ms, "trackPullInMs", 1000), pick(handover_ms, "trackHandOverMs", 100), 0)


class LockParams(C.Structure):
    """sgx_lock_params: the C/N0 and lock-detector parameters of sgx_track_quality (32 bytes)."""
    _fields_ = [("T", C.c_double), ("cno_min", C.c_double), ("carr_lock_min", C.c_double), ("window", C.c_int32),
                ("max_fail", C.c_int32)]


class ReplayBlock(C.Structure):
    """sgx_replay_block: one block of a tracked channel as sgx_replay_state rebuilds it (48 bytes)."""
    _fields_ = [("start", C.c_int64), ("rem_code", C.c_double), ("rem_carr", C.c_double), ("step", C.c_double),
                ("carr_freq", C.c_double), ("blk", C.c_int32), ("reserved", C.c_int32)]


class RequantStats(C.Structure):
    """sgx_requant_stats: the statistics of a window of int16 / float32 elements (sgx_requant_stats_of, 40 bytes)."""
    _fields_ = [("n_finite", C.c_int64), ("n_nonfinite", C.c_int64), ("max_abs", C.c_double), ("sum", C.c_double),
                ("sum_sq", C.c_double)]


class CondStats(C.Structure):
    """sgx_cond_stats: the statistics of one block of the conditioning stage (sgx_cond_block_stats, 64 bytes)."""
    _fields_ = [(k, C.c_int64) for k in ("n", "kept", "dc0", "dc1", "p_kept", "p_all", "e_max", "reserved")]


class CondEntry(C.Structure):
    """sgx_cond_entry: DC, gain and blanking threshold of one block (sgx_cond_plan -> sgx_if_condition, 24 bytes)."""
    _fields_ = [("dc0", C.c_int32), ("dc1", C.c_int32), ("mult", C.c_int32), ("shift", C.c_int32), ("theta", C.c_int64)]


COND_STATS_DTYPE = np.dtype([(k, "<i8") for k in ("n", "kept", "dc0", "dc1", "p_kept", "p_all", "e_max", "reserved")])
COND_PLAN_DTYPE = np.dtype([("dc0", "<i4"), ("dc1", "<i4"), ("mult", "<i4"), ("shift", "<i4"), ("theta", "<i8")])
COND_OFFSET_BINARY = 1
REPLAY_MAX_TAPS = 64
REPLAY_STATE_DTYPE = np.dtype([("start", "<i8"), ("rem_code", "<f8"), ("rem_carr", "<f8"), ("step", "<f8"),
                               ("carr_freq", "<f8"), ("blk", "<i4"), ("reserved", "<i4")])

class ExciseInfo(C.Structure):
    """sgx_excise_info: what sgx_if_excise and sgx_excise_host count."""
    _fields_ = [(k, C.c_int64) for k in ("segments", "bins_cut", "segments_cut", "clipped")]


# every symbol include/sgx.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_PROTOS = {
    "sgx_version": (C.c_char_p, []),
    "sgx_last_error": (C.c_int, [C.c_char_p, C.c_size_t]),
    "sgx_samples_per_code": (C.c_int, [C.POINTER(Settings), C.POINTER(C.c_int64)]),
    "sgx_generate_ca_code": (C.c_int, [C.c_int32, _P]),
    "sgx_make_ca_table": (C.c_int, [C.POINTER(Settings), _P]),
    "sgx_calc_loop_coef": (C.c_int, [C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double),
                                     C.POINTER(C.c_double)]),
    "sgx_trk_math_eval": (C.c_int, [C.c_int32, C.c_double, C.c_double, _P]),
    "sgx_trk_math_eval_batch": (C.c_int, [C.c_int32, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "sgx_trk_math_eval_device": (C.c_int, [_P, C.c_int32, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "sgx_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "sgx_ctx_create": (C.c_int, [C.POINTER(Settings), C.c_int, C.POINTER(_P)]),
    "sgx_ctx_create_prio": (C.c_int, [C.POINTER(Settings), C.c_int, C.c_int, C.POINTER(_P)]),
    "sgx_ctx_destroy": (C.c_int, [_P]),
    "sgx_ctx_sync": (C.c_int, [_P]),
    "sgx_get_timing": (C.c_int, [_P, C.POINTER(Timing)]),
    "sgx_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(_P)]),
    "sgx_host_free": (C.c_int, [_P]),
    "sgx_if_upload": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(_P)]),
    "sgx_if_upload_file": (C.c_int, [_P, C.c_char_p, C.c_uint64, C.c_size_t, C.POINTER(_P)]),
    "sgx_if_open_file": (C.c_int, [_P, C.c_char_p, C.c_uint64, C.c_size_t, C.POINTER(_P)]),
    "sgx_if_wait": (C.c_int, [_P, _P, C.c_size_t]),
    "sgx_if_synth": (C.c_int, [_P, C.POINTER(Scene), C.c_uint64, C.c_size_t, C.POINTER(_P)]),
    "sgx_if_download": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P]),
    "sgx_if_length": (C.c_int, [_P, C.POINTER(C.c_size_t)]),
    "sgx_if_free": (C.c_int, [_P, _P]),
    "sgx_acquire": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_int32, C.c_int32, C.c_int32,
                              _P, _P, _P, _P, _P]),
    "sgx_acquire_f64": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "sgx_acquire_coherent": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_int32, C.POINTER(AcqParams),
                                       _P, _P, _P, _P, _P]),
    "sgx_acquire_coherent_f64": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_int32, C.POINTER(AcqParams), _P, _P, _P, _P, _P]),
    "sgx_acquire_coherent_plan": (C.c_int, [C.POINTER(Settings), C.POINTER(AcqParams)] + [C.POINTER(C.c_int32)] * 5),
    "sgx_acquire_begin": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_int32, C.c_int32, C.c_int32]),
    "sgx_acquire_end": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "sgx_track_chained": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P,
                                    C.POINTER(C.c_int32)]),
    "sgx_track": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, C.c_int32, _P, _P]),
    "sgx_track_coherent": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, C.c_int32, C.POINTER(CohParams), _P, _P, _P, _P, _P, _P]),
    "sgx_track_ex": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32]),
    "sgx_track_plan": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sgx_acquire_plan": (C.c_int, [C.c_int32] * 6 + [C.POINTER(C.c_int32)] * 4),
    "sgx_acquire_plan_limits": (C.c_int, [C.POINTER(C.c_int32)] * 2),
    "sgx_acquire_fft_length": (C.c_int, [C.c_int64, C.POINTER(C.c_int64)]),
    "sgx_acquire_fft_passes": (C.c_int, [C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sgx_fft_run_passes": (C.c_int, [_P, C.c_int64, C.c_int32, _P, C.c_int64, _P, C.c_int32, _P, C.c_int32, C.c_int32,
                                     C.c_int32, _P, C.c_int64, _P, _P, _P]),
    "sgx_stream_rates": (C.c_int, [_P, C.c_size_t, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "sgx_probe_stats": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_double, _P, _P, _P, C.POINTER(C.c_int32)]),
    "sgx_probe_waterfall": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_double, C.c_int32, C.c_int32, C.c_size_t,
                                      _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    "sgx_waterfall_plan": (C.c_int, [C.c_size_t, C.c_int32, C.c_int32, C.c_size_t, C.POINTER(C.c_int64)]),
    "sgx_waterfall_host": (C.c_int, [_P, C.c_size_t, C.c_double, C.c_int32, C.c_int32, C.c_size_t, _P, _P]),
    "sgx_waterfall_timing": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "sgx_excise_plan": (C.c_int, [C.c_size_t, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "sgx_if_excise": (C.c_int, [_P, _P, C.c_int32, C.c_double, C.c_int32, C.POINTER(_P), C.POINTER(ExciseInfo), _P]),
    "sgx_excise_host": (C.c_int, [_P, C.c_size_t, C.c_int32, C.c_double, C.c_int32, _P, C.POINTER(ExciseInfo), _P]),
    "sgx_excise_host_spectra": (C.c_int, [_P, C.c_size_t, C.c_int32, _P]),
    "sgx_excise_timing": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "sgx_find_preambles": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "sgx_nav_parity_check": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "sgx_track_quality": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.POINTER(LockParams), _P, _P, _P,
                                    _P]),
    "sgx_replay_state": (C.c_int, [C.POINTER(Settings), C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, C.c_int64, C.c_int64, _P]),
    "sgx_track_replay": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, _P]),
    "sgx_replay_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sgx_cancel_design": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    "sgx_if_cancel": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, C.POINTER(_P),
                                C.POINTER(C.c_int64)]),
    "sgx_cancel_host": (C.c_int, [C.POINTER(Settings), _P, C.c_size_t, C.c_int64, _P, C.c_int32, C.c_int32, _P, _P,
                                  C.c_int32, _P, _P, C.POINTER(C.c_int64)]),
    "sgx_cancel_timing": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "sgx_notch_design": (C.c_int, [C.POINTER(Settings), _P, _P, C.c_int32, C.c_double, C.c_double, C.c_int32, _P,
                                   C.POINTER(C.c_int32), _P, _P, C.POINTER(C.c_int32)]),
    "sgx_if_filter": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.POINTER(_P)]),
    "sgx_filter_timing": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "sgx_iq_design": (C.c_int, [C.c_int32, _P, C.POINTER(C.c_int32)]),
    "sgx_if_from_iq": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    "sgx_iq_timing": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "sgx_iq_tile": (C.c_int, [C.POINTER(C.c_int32)]),
    "sgx_requant_stats_of": (C.c_int, [_P, _P, C.c_int32, C.c_size_t, C.c_size_t, C.POINTER(RequantStats)]),
    "sgx_requant_gain": (C.c_int, [C.POINTER(RequantStats), C.c_int32, C.c_double, C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "sgx_if_requantize": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.POINTER(_P),
                                    C.POINTER(C.c_int64)]),
    "sgx_requant_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sgx_requant_tile": (C.c_int, [C.POINTER(C.c_int32)]),
    "sgx_cond_block_stats": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_size_t,
                                       C.POINTER(C.c_size_t)]),
    "sgx_cond_plan": (C.c_int, [_P, C.c_size_t, C.c_int32, C.c_int32, C.c_double, C.c_double, _P]),
    "sgx_if_condition": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_size_t, C.c_int32,
                                   C.POINTER(_P), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sgx_cond_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sgx_cond_tile": (C.c_int, [C.POINTER(C.c_int32)]),
    "sgx_unpack_table": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P]),
    "sgx_if_unpack": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(_P), _P]),
    "sgx_unpack_timing": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "sgx_unpack_tile": (C.c_int, [C.POINTER(C.c_int32)]),
    "sgx_decim_design": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_double, _P,
                                   C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(C.c_int32)]),
    "sgx_if_decimate": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P),
                                  C.POINTER(C.c_int64)]),
    "sgx_decim_timing": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "sgx_decim_tile": (C.c_int, [C.POINTER(C.c_int32)]),
    "sgx_resamp_design": (C.c_int, [C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _P,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "sgx_if_resample": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P),
                                  C.POINTER(C.c_int64)]),
    "sgx_resamp_timing": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "sgx_resamp_tile": (C.c_int, [C.POINTER(C.c_int32)]),
    "sgx_array_stats": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "sgx_array_stats_timing": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "sgx_array_stats_tile": (C.c_int, [C.POINTER(C.c_int32)]),
    "sgx_array_design": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _P,
                                   C.POINTER(C.c_int32), _P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "sgx_if_combine": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P),
                                 C.POINTER(C.c_int64)]),
    "sgx_combine_timing": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "sgx_combine_tile": (C.c_int, [C.POINTER(C.c_int32)]),
    "sgx_array_block_stats": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _P]),
    "sgx_array_block_stats_timing": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "sgx_array_design_blocks": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_double, C.c_double, _P, C.POINTER(C.c_int32), _P, _P, _P, _P]),
    "sgx_if_combine_blocks": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                        C.c_int32, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "sgx_combine_blocks_timing": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "sgx_check_t": (C.c_int, [C.c_double, _P]),
    "sgx_e_r_corr": (C.c_int, [C.c_double, _P, _P]),
    "sgx_togeod": (C.c_int, [C.c_double] * 5 + [_P, _P, _P]),
    "sgx_topocent": (C.c_int, [_P] * 5),
    "sgx_tropo": (C.c_int, [C.c_double] * 8 + [_P]),
    "sgx_satpos": (C.c_int, [C.c_double, _P, C.c_int32, _P, _P, _P]),
    "sgx_least_square_pos": (C.c_int, [_P, _P, C.c_int32, C.c_double, C.c_int32, _P, _P, _P, _P, _P]),
    "sgx_cart2geo": (C.c_int, [C.c_double] * 3 + [C.c_int32, _P, _P, _P]),
    "sgx_find_utm_zone": (C.c_int, [C.c_double, C.c_double, _P]),
    "sgx_cart2utm": (C.c_int, [C.c_double] * 3 + [C.c_int32, _P, _P, _P]),
    "sgx_ephemeris": (C.c_int, [_P, C.c_int32, C.c_uint8, _P, C.POINTER(C.c_int64)]),
    "sgx_pseudoranges": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_double,
                                   C.c_double, _P]),
    "sgx_nav_bits": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.POINTER(C.c_int32)]),
    "sgx_post_navigate": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, _P, C.c_int64, C.c_int64,
                                    C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32,
                                    _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int32), _P]),
    "sgx_comm_unique_id": (C.c_int, [_P]),
    "sgx_comm_create": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.POINTER(_P)]),
    "sgx_comm_allgather": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "sgx_comm_destroy": (C.c_int, [_P]),
    "sgx_acquire_sharded": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32,
                                      C.c_int32, _P, _P, _P, _P, _P]),
}
SYMBOLS = tuple(sorted(_PROTOS))

_lib = None


def lib():
    """Load libsgx.so (built in-tree by build.py / __graft_entry__.build). Raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libsgx.so is not built (%s missing): run `python __graft_entry__.py` or "
                              "`python softgnss-python_amd/build.py`; there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            f = getattr(L, name)   # AttributeError if the library lacks a declared symbol
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def last_error():
    buf = C.create_string_buffer(512)
    lib().sgx_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def check(code):
    if code != SGX_OK:
        msg = last_error()
        if code == SGX_E_INDEX:
            raise IndexError(msg)          # the reference raises IndexError here (acquisition.py:152-162)
        if code == SGX_E_SILENT:
            raise SilentChannelError(msg)  # the reference raises ValueError here (tracking.py:148-151)
        raise SgxError(code, msg)


def settings_struct(s):
    """POD mirror of a Settings-like object (attribute names of reference initialize.py:85-173)."""
    return Settings(float(s.samplingFreq), float(s.IF), float(s.codeFreqBasis), float(s.acqSearchBand),
                    float(s.acqThreshold), float(s.dllDampingRatio), float(s.dllNoiseBandwidth),
                    float(s.dllCorrelatorSpacing), float(s.pllDampingRatio), float(s.pllNoiseBandwidth),
                    int(s.skipNumberOfBytes), int(s.codeLength), int(s.numberOfChannels))


def track_plan(settings, data_type=0, n_channels=8, n_cus=256, float_in_range=False):
    """(kernel, members per channel) sgx_track_ex would run for these settings, sample type and channel count on a device
    with n_cus compute units - the host's one selection rule (csrc/sgx_trk.hip); needs no GPU."""
    st = settings_struct(settings)
    k, mbr = C.c_int32(0), C.c_int32(0)
    check(lib().sgx_track_plan(C.byref(st), int(data_type), int(n_channels), int(n_cus), 1 if float_in_range else 0,
                               C.byref(k), C.byref(mbr)))
    return k.value, mbr.value


def trk_math_eval(fn, a, b=None, c=None, d=None, ctx=None):
    """(out0, out1): function fn of the tracking chain's arithmetic (include/sgx.h: sgx_trk_math_eval_batch) on every
    element of the float64 operand arrays, on the host - or, with ctx (a Context), on its device as the device compiles it
    (sgx_trk_math_eval_device, which also knows the device-only functions)."""
    ops = [None if x is None else np.ascontiguousarray(x, dtype=np.float64).ravel() for x in (a, b, c, d)]
    n = ops[0].size
    for x in ops[1:]:
        if x is not None and x.size != n:
            raise ValueError("operands of %d and %d elements" % (n, x.size))
    out0, out1 = np.zeros(n), np.zeros(n)
    ptrs = [None if x is None else _ptr(x) for x in ops] + [_ptr(out0), _ptr(out1)]
    if ctx is None:
        check(lib().sgx_trk_math_eval_batch(int(fn), n, *ptrs))
    else:
        check(lib().sgx_trk_math_eval_device(ctx._h, int(fn), n, *ptrs))
    return out0, out1


def acquire_plan(n_prn=32, n_bins=29, n_blocks=2, noncoh=False, chunk_rows=0, max_queues=2):
    """(PRNs per chunk, runs of Doppler bins per PRN, bins per run, queues): how sgx_acquire cuts the correlation batch -
    the host's one rule (csrc/sgx_acq.hip: acq_plan); needs no GPU."""
    v = [C.c_int32(0) for _ in range(4)]
    check(lib().sgx_acquire_plan(int(n_prn), int(n_bins), int(n_blocks), 1 if noncoh else 0, int(chunk_rows), int(max_queues),
                                 *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def acquire_coherent_plan(settings, coherent_ms=1, n_windows=2, noncoh=False, bin_step_hz=None):
    """The coherent search sgx_acquire_coherent runs for these settings, for 32 PRNs (include/sgx.h); needs no GPU.
    Returns dict(n_bins, n_phi, path ('shift' or 'direct'), prn_chunk, bin_runs)."""
    st = settings_struct(settings)
    pa = acq_params(coherent_ms, n_windows, noncoh, bin_step_hz)
    v = [C.c_int32(0) for _ in range(5)]
    check(lib().sgx_acquire_coherent_plan(C.byref(st), C.byref(pa), *[C.byref(x) for x in v]))
    return dict(n_bins=v[0].value, n_phi=v[1].value, path="shift" if v[2].value == 1 else "direct",
                prn_chunk=v[3].value, bin_runs=v[4].value)


def acquire_plan_limits():
    """(default chunk rows, largest batch of rows per launch) of csrc/sgx_acq.hip's chunk rule."""
    a, b = C.c_int32(0), C.c_int32(0)
    check(lib().sgx_acquire_plan_limits(C.byref(a), C.byref(b)))
    return a.value, b.value


def acquire_fft_length(n_code):
    """The transform length sgx_acquire's search runs on for samplesPerCode = n_code: n_code where it factors into 2..31,
    else the padded length (>= 2 n_code - 1) its circular correlation is embedded in (include/sgx.h); needs no GPU."""
    m = C.c_int64(0)
    check(lib().sgx_acquire_fft_length(int(n_code), C.byref(m)))
    return m.value


FFT_MAX_PASSES = 32


def acquire_fft_passes(n_code):
    """The radix passes sgx_acquire's search runs for samplesPerCode = n_code (include/sgx.h); needs no GPU.  Returns
    dict(length, radices, tpb (workgroup width per pass), last_pass_blocks)."""
    rad, tpb = (C.c_int32 * FFT_MAX_PASSES)(), (C.c_int32 * FFT_MAX_PASSES)()
    k, blocks, length = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    check(lib().sgx_acquire_fft_passes(int(n_code), rad, C.byref(k), C.byref(length), C.byref(blocks), tpb))
    return dict(length=length.value, radices=list(rad[:k.value]), tpb=list(tpb[:k.value]), last_pass_blocks=blocks.value)


def _c128(a, n):
    a = np.ascontiguousarray(a, dtype=np.complex128)
    if a.ndim != 2 or a.shape[1] != n:
        raise ValueError("rows of %d complex128 expected, got shape %s" % (n, a.shape))
    return a


def fft_forward(ctx, rows, nonzero_len=None):
    """DFT of every row of `rows` [rows][n] by the radix-pass kernels (sgx_fft_run_passes, plain form), the input taken
    as zero from element nonzero_len on.  ctx: a device context handle."""
    x = _c128(rows, np.shape(rows)[1])
    n = x.shape[1]
    out = np.empty_like(x)
    check(lib().sgx_fft_run_passes(ctx, n, x.shape[0], x.ctypes.data, n if nonzero_len is None else int(nonzero_len),
                                   None, 0, None, 0, 1, 0, None, 0, out.ctypes.data, None, None))
    return out


def fft_fused(ctx, mul_x, mul_f, rows, rows_per_prn=1, prn_base=0, row_map=None, n_valid=0, want_rows=False):
    """The fused correlation passes on spectra mul_x [n_x][n] and mul_f [n_f][n] (sgx_fft_run_passes, fused form): row r
    transforms conj(mul_x[b]) * mul_f[p], (b, p) from row_map [rows][2] or the regular layout.  Returns (max, arg) per
    row over the outputs below n_valid (0: all), or the rows themselves with want_rows."""
    n = np.shape(mul_x)[1]
    x, f = _c128(mul_x, n), _c128(mul_f, n)
    rm = None
    if row_map is not None:
        rm = np.ascontiguousarray(row_map, dtype=np.int32)
        if rm.shape != (int(rows), 2):
            raise ValueError("row_map of shape (%d, 2) expected" % int(rows))
    args = (ctx, n, int(rows), None, n, x.ctypes.data, x.shape[0], f.ctypes.data, f.shape[0], int(rows_per_prn),
            int(prn_base), None if rm is None else rm.ctypes.data, int(n_valid))
    if want_rows:
        out = np.empty((int(rows), n), dtype=np.complex128)
        check(lib().sgx_fft_run_passes(*args, out.ctypes.data, None, None))
        return out
    mx, arg = np.empty(int(rows), dtype=np.float64), np.empty(int(rows), dtype=np.int32)
    check(lib().sgx_fft_run_passes(*args, None, mx.ctypes.data, arg.ctypes.data))
    return mx, arg


def scene_struct(scene):
    sc = Scene()
    sc.seed = scene.seed
    sc.n_sats = len(scene.sats)
    for i, s in enumerate(scene.sats):
        sc.sats[i] = Sat(s["code_fcw"], s["code_c0"], s["nav_seed"], s["car_fcw"], s["car_ph0"], s["prn"],
                         s["amp"])
    for i in range(256):
        sc.cos_lut[i] = int(scene.cos_lut[i])
    tab = getattr(scene, "nav_bits", None)
    sc.nav_mode = 0 if tab is None else 1
    if tab is not None:
        for i in range(len(scene.sats)):
            packed = np.packbits(np.asarray(tab[i], dtype=np.uint8), bitorder="little")
            for j in range(256):
                sc.nav_bits[i][j] = int(packed[j])
    return sc


class _Pinned(object):
    """Owner of one pinned host allocation.  `busy` is set while a numpy array handed out by pinned_empty() is alive
    (cleared by a weakref finalizer on the ctypes buffer the array is built on)."""

    def __init__(self, nbytes):
        self.ptr = _P()
        check(lib().sgx_host_alloc(int(nbytes), C.byref(self.ptr)))
        self.nbytes = int(nbytes)
        self.busy = False

    def __del__(self):
        try:
            if self.ptr:
                lib().sgx_host_free(self.ptr)
        except Exception:
            pass


_pinned_pool = []   # pinning is slow (ms per 30 MB): allocations whose arrays have died are reused
_pinned_lock = threading.RLock()   # re-entrant: a finalizer may run (cyclic GC) while pinned_empty() holds it


def _pinned_release(own):
    with _pinned_lock:
        own.busy = False


def pinned_empty(shape, dtype=np.float64):
    """numpy array in pinned host memory (falls back to a pageable array if pinning fails)."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    own = None
    with _pinned_lock:
        for cand in _pinned_pool:
            if cand.nbytes >= n and not cand.busy:
                own = cand
                break
        if own is not None:
            own.busy = True
    if own is None:
        try:
            own = _Pinned(max(n, 1))
        except Exception:
            return np.empty(shape, dtype=dtype)
        own.busy = True
        with _pinned_lock:
            _pinned_pool.append(own)
            while len(_pinned_pool) > 8:
                # drop an idle allocation (a busy one stays alive through its array even when it leaves the pool)
                idle = [c for c in _pinned_pool if not c.busy and c is not own]
                _pinned_pool.remove(idle[0] if idle else _pinned_pool[0])
    buf = (C.c_char * own.nbytes).from_address(own.ptr.value)
    buf._owner = own                       # ctypes object keeps the owner, numpy keeps the ctypes object
    weakref.finalize(buf, _pinned_release, own)   # every view of the array holds `buf` through .base
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def lock_params(settings):
    """LockParams from Settings' lock-detector attributes (cnoInterval, cnoThreshold, carrLockThreshold, maxLockFail)."""
    return LockParams(float(settings.codeLength) / float(settings.codeFreqBasis), float(settings.cnoThreshold),
                      float(settings.carrLockThreshold), int(round(float(settings.cnoInterval))),
                      int(settings.maxLockFail))


def _chan_array(chans):
    arr = (ChanInit * len(chans))()
    for i, (prn, f, cp) in enumerate(chans):
        arr[i] = ChanInit(float(f), float(cp), int(prn), 0)
    return arr


def _series3(series, n):
    a = np.ascontiguousarray(series, dtype=np.float64)
    if a.ndim != 3 or a.shape[0] != n or a.shape[1] != NUM_SERIES:
        raise ValueError("expected a [%d, %d, ms] series array, got shape %r" % (n, NUM_SERIES, a.shape))
    return a


def replay_state(settings, chans, series, ms_done=None, data_type=DT_INT8, rec_file_offset=0, rec_bytes=-1):
    """The per-block state of tracked channels (sgx_replay_state; needs no GPU).  chans: (prn, acquiredFreq, codePhase)
    per channel, series: float64[n_ch, 13, ms] of track(); rec_bytes < 0: the record's extent is not checked.  Returns a
    structured array [n_ch, ms] with the fields start, rem_code, rem_carr, step, carr_freq, blk."""
    n = len(chans)
    a = _series3(series, n)
    ms = a.shape[2]
    done, done_p = _ms_done(ms_done, n)
    st = settings_struct(settings)
    out = np.zeros((n, ms), dtype=REPLAY_STATE_DTYPE)
    check(lib().sgx_replay_state(C.byref(st), int(data_type), C.cast(_chan_array(chans), _P), n, ms,
                                 done_p, _ptr(a), int(rec_file_offset), int(rec_bytes), _ptr(out)))
    return out


CANCEL_MAX_CHANNELS, CANCEL_MAX_SMOOTH = 32, 41


def _amp3(amp, n, ms):
    a = np.ascontiguousarray(amp, dtype=np.float64)
    if a.shape != (n, ms, 2):
        raise ValueError("expected a [%d, %d, 2] amplitude array, got shape %r" % (n, ms, a.shape))
    return a


def cancel_design(series, state, ms_done=None, smooth=1):
    """float64[n_ch, ms, 2]: the amplitude pair (aI, aQ) of every block of tracked channels from their prompt sums
    (sgx_cancel_design; needs no GPU).  series: float64[n_ch, 13, ms] of track(), state: what replay_state made of it,
    smooth: the odd number of neighbouring blocks, 1 .. 41, a pair is averaged over (data-bit signs aligned)."""
    st = np.ascontiguousarray(state, dtype=REPLAY_STATE_DTYPE)
    n = st.shape[0]
    a = _series3(series, n)
    ms = a.shape[2]
    if st.shape != (n, ms):
        raise ValueError("the state has shape %r, the series %r" % (st.shape, a.shape))
    done, done_p = _ms_done(ms_done, n)
    out = np.zeros((n, ms, 2))
    check(lib().sgx_cancel_design(_ptr(a), _ptr(st), n, ms, done_p, int(smooth), _ptr(out)))
    return out


def cancel_host(settings, x, chans, series, amp, ms_done=None, rec_file_offset=0, data_type=DT_INT8):
    """(y int8, clipped) of sgx_cancel_host: the cancellation kernel's work sample by sample on the host; test
    infrastructure, needs no GPU.  x: the record, the file's bytes from rec_file_offset on."""
    a = np.ascontiguousarray(x, dtype=np.int8).ravel()
    n = len(chans)
    ser = _series3(series, n)
    ms = ser.shape[2]
    am = _amp3(amp, n, ms)
    done, done_p = _ms_done(ms_done, n)
    st = settings_struct(settings)
    y, clipped = np.zeros(a.size, dtype=np.int8), C.c_int64(0)
    check(lib().sgx_cancel_host(C.byref(st), _ptr(a), a.size, int(rec_file_offset), C.cast(_chan_array(chans), _P), n, ms,
                                done_p, _ptr(ser), int(data_type), _ptr(am), _ptr(y), C.byref(clipped)))
    return y, int(clipped.value)


FILTER_MAX_TAPS = 4095
NOTCH_MAX_LINES = 8


def notch_design(settings, f_mhz, pxx, threshold_db=8.0, width_hz=80e3, n_taps=1025):
    """Lines of a one-sided PSD and the integer notch that removes them (sgx_notch_design; needs no GPU).  f_mhz, pxx: the
    spectrum as probe_stats gives it.  Returns (taps int16[n_taps], shift, lines): lines is a list of (centre Hz, width Hz)
    in ascending frequency, at most 8; with no line the taps are the identity filter."""
    f = np.ascontiguousarray(f_mhz, dtype=np.float64).ravel()
    p = np.ascontiguousarray(pxx, dtype=np.float64).ravel()
    if f.size != p.size:
        raise ValueError("f_mhz has %d entries, pxx %d" % (f.size, p.size))
    st = settings_struct(settings)
    taps = np.zeros(max(int(n_taps), 1), dtype=np.int16)
    hz, wd = np.zeros(NOTCH_MAX_LINES), np.zeros(NOTCH_MAX_LINES)
    shift, n = C.c_int32(0), C.c_int32(0)
    check(lib().sgx_notch_design(C.byref(st), _ptr(f), _ptr(p), f.size, float(threshold_db), float(width_hz), int(n_taps),
                                 _ptr(taps), C.byref(shift), _ptr(hz), _ptr(wd), C.byref(n)))
    return taps, shift.value, [(float(hz[i]), float(wd[i])) for i in range(n.value)]


WATERFALL_MIN_SEGMENT, WATERFALL_MAX_SEGMENT = 256, 16384


def waterfall_plan(n, nperseg, noverlap, slice_len):
    """The number of slices Context.waterfall keeps of a window of n samples (sgx_waterfall_plan; needs no GPU).
    ValueError for what the monitor refuses: a segment length that is no power of two in 256 .. 16384, an overlap outside
    [0, nperseg), a slice shorter than a segment or longer than 2^32 samples, a window shorter than one segment."""
    ns = C.c_int64(0)
    rc = lib().sgx_waterfall_plan(max(int(n), 0), int(nperseg), int(noverlap), max(int(slice_len), 0), C.byref(ns))
    if rc in (SGX_E_ARG, SGX_E_RANGE):
        raise ValueError(last_error())
    check(rc)
    return int(ns.value)


def waterfall_host(x, fs_mhz, nperseg=16384, noverlap=1024, slice_len=None):
    """(pxx float64[n_slices, bins], n_segments int64[n_slices]) of sgx_waterfall_host: the monitor's spectra of the window x
    by the kernels' work items in a host loop; test infrastructure, needs no GPU.  ValueError as waterfall_plan."""
    a = np.ascontiguousarray(x, dtype=np.int8).ravel()
    S = a.size if slice_len is None else int(slice_len)
    ns = waterfall_plan(a.size, nperseg, noverlap, S)
    pxx, nseg = np.zeros((ns, int(nperseg) // 2 + 1)), np.zeros(ns, dtype=np.int64)
    check(lib().sgx_waterfall_host(_ptr(a), a.size, float(fs_mhz), int(nperseg), int(noverlap), S, _ptr(pxx), _ptr(nseg)))
    return pxx, nseg


EXCISE_MIN_SEGMENT, EXCISE_MAX_SEGMENT, EXCISE_MAX_PASSES = 64, 1024, 8


def excise_plan(n, N):
    """(segments J, segments of one tile) of the excision of a record of n samples at segment length N (sgx_excise_plan;
    needs no GPU).  ValueError for an N that is no power of two in 64 .. 1024 and for an empty record."""
    J, S = C.c_int64(0), C.c_int32(0)
    rc = lib().sgx_excise_plan(max(int(n), 0), int(N), C.byref(J), C.byref(S))
    if rc == SGX_E_ARG:
        raise ValueError(last_error())
    check(rc)
    return int(J.value), int(S.value)


def _excise_info(info, per_segment):
    return dict(segments=int(info.segments), bins_cut=int(info.bins_cut), segments_cut=int(info.segments_cut),
                clipped=int(info.clipped), cut_per_segment=per_segment)


def excise_host(x, N=256, threshold=8.0, passes=3):
    """(y int8, info) of sgx_excise_host: the excision kernel's work items in a host loop; test infrastructure, needs no
    GPU.  info as Context.excise_record's.  SgxError for what the library refuses."""
    a = np.ascontiguousarray(x, dtype=np.int8).ravel()
    y = np.zeros(a.size, dtype=np.int8)
    ok = EXCISE_MIN_SEGMENT <= int(N) <= EXCISE_MAX_SEGMENT      # (what is out of range is the library's to refuse)
    per = np.zeros(-(-a.size // (int(N) // 2)) + 1 if ok else 1, dtype=np.uint16)
    info = ExciseInfo()
    check(lib().sgx_excise_host(_ptr(a), a.size, int(N), float(threshold), int(passes), _ptr(y), C.byref(info), _ptr(per)))
    return y, _excise_info(info, per[:info.segments])


def excise_host_spectra(x, N=256):
    """complex128[J, N/2 + 1]: the bins of the windowed segments as the host items compute them (sgx_excise_host_spectra)."""
    a = np.ascontiguousarray(x, dtype=np.int8).ravel()
    J = excise_plan(a.size, N)[0]
    out = np.zeros((J, int(N) // 2 + 1), dtype=np.complex128)
    check(lib().sgx_excise_host_spectra(_ptr(a), a.size, int(N), _ptr(out)))
    return out


class Waterfall(object):
    """What Context.waterfall returns.  f[bins] (MHz), pxx[n_slices, bins], hold[bins] (the maximum over the slices),
    moments int64[n_slices, 4] (count, sum x, sum x^2, sum x^4), hist int64[n_slices, 256] (-128 in bin 0), n_segments
    int64[n_slices]; and, in float64 from those integers, per slice: mean, rms, kurtosis (excess, m4 / m2^2 - 3 about the
    mean; 0 for a constant slice) and clip_share (the share of the samples on -128, -127 or +127)."""

    def __init__(self, f, pxx, hold, moments, hist, n_segments, slice_len):
        self.f, self.pxx, self.hold, self.moments, self.hist, self.n_segments = f, pxx, hold, moments, hist, n_segments
        self.slice_len = int(slice_len)
        n = moments[:, 0].astype(np.float64)
        v = np.arange(-128, 128, dtype=np.int64)
        self.mean = moments[:, 1] / n
        e2, e3, e4 = moments[:, 2] / n, (hist * v ** 3).sum(axis=1) / n, moments[:, 3] / n
        m2 = e2 - self.mean * self.mean
        m4 = e4 - 4.0 * self.mean * e3 + 6.0 * self.mean * self.mean * e2 - 3.0 * self.mean ** 4
        self.rms = np.sqrt(e2)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.kurtosis = np.where(m2 > 0, m4 / (m2 * m2) - 3.0, 0.0)
        self.clip_share = (hist[:, 0] + hist[:, 1] + hist[:, 255]) / n

    def arrays(self):
        """The arrays by name, as --monitor-out saves them."""
        return dict((k, getattr(self, k)) for k in ("f", "pxx", "hold", "moments", "hist", "n_segments", "mean", "rms",
                                                    "kurtosis", "clip_share"))


IQ_MAX_TAPS = 255
IQ_Q_FIRST, IQ_OFFSET_BINARY = 1, 2


def iq_design(n_taps=63):
    """(taps int16[n_taps], shift): the half-band interpolation filter of the I/Q converter (sgx_iq_design; needs no GPU)."""
    taps = np.zeros(max(int(n_taps), 1), dtype=np.int16)
    shift = C.c_int32(0)
    check(lib().sgx_iq_design(int(n_taps), _ptr(taps), C.byref(shift)))
    return taps, shift.value


def _tile(name):
    """What one workgroup of a record stage makes, as its sgx_*_tile getter reports it."""
    t = C.c_int32(0)
    check(getattr(lib(), name)(C.byref(t)))
    return t.value


def iq_tile():
    """Output bytes one workgroup of the I/Q converter makes: its tile seams lie at the multiples."""
    return _tile("sgx_iq_tile")


REQUANT_SCALE_MIN, REQUANT_SCALE_MAX = 2.0 ** -100, 2.0 ** 100


def requant_type(dtype):
    """(sgx data_type, bytes per element) of a sample type the requantiser reads: int16 or float32."""
    dt = np.dtype(dtype)
    if dt == np.dtype(np.int16):
        return DT_INT16, 2
    if dt == np.dtype(np.float32):
        return DT_FLOAT32, 4
    raise ValueError("the requantiser reads int16 and float32 records, not %r" % (dtype,))


def requant_gain(stats, dtype, target_rms=12.0):
    """(mult, shift, scale): the fixed gain that brings a record with these statistics (the dict of Context.requant_stats,
    or anything with n_finite and sum_sq) to target_rms, in (0, 127] (sgx_requant_gain; exact host code, needs no GPU).
    int16 records are requantised with mult / 2^shift, float32 records with the float32 scale."""
    get = stats.get if isinstance(stats, dict) else (lambda k, d=0: getattr(stats, k, d))
    st = RequantStats(int(get("n_finite", 0)), int(get("n_nonfinite", 0)), float(get("max_abs", 0.0)),
                      float(get("sum", 0.0)), float(get("sum_sq", 0.0)))
    m, sh, sc = C.c_int32(0), C.c_int32(0), C.c_float(0)
    check(lib().sgx_requant_gain(C.byref(st), requant_type(dtype)[0], float(target_rms), C.byref(m), C.byref(sh),
                                 C.byref(sc)))
    return m.value, sh.value, np.float32(sc.value)


def requant_tile():
    """Output bytes (= elements) one workgroup of the requantiser makes: its tile seams lie at the multiples."""
    return _tile("sgx_requant_tile")


def cond_type(dtype, offset_binary=False):
    """(sgx data_type, bytes per element, flags) of a sample type the conditioning stage reads: int8, uint8 (offset binary:
    element = byte - 128) or int16."""
    dt = np.dtype(dtype)
    if dt == np.dtype(np.uint8):
        return DT_INT8, 1, COND_OFFSET_BINARY
    if dt == np.dtype(np.int8):
        return DT_INT8, 1, COND_OFFSET_BINARY if offset_binary else 0
    if dt == np.dtype(np.int16):
        return DT_INT16, 2, COND_OFFSET_BINARY if offset_binary else 0   # (the library refuses the flag with int16)
    raise ValueError("the conditioning stage reads int8, uint8 and int16 records, not %r" % (dtype,))


def cond_plan(stats, lanes, blank_q4, target_rms=12.0, agc_blocks=32.0):
    """The per-block plan of the conditioning stage (sgx_cond_plan; exact host code, needs no GPU): stats, the
    COND_STATS_DTYPE array of Context.cond_stats, smoothed over agc_blocks blocks into a COND_PLAN_DTYPE array of
    (dc0, dc1, mult, shift, theta) per block."""
    st = np.ascontiguousarray(stats, dtype=COND_STATS_DTYPE).ravel()
    plan = np.zeros(st.size, dtype=COND_PLAN_DTYPE)
    check(lib().sgx_cond_plan(_ptr(st), st.size, int(lanes), int(blank_q4), float(target_rms), float(agc_blocks),
                              _ptr(plan)))
    return plan


def cond_tile():
    """Frames one workgroup of the conditioning kernel makes: its tile seams lie at the multiples."""
    return _tile("sgx_cond_tile")


UNPACK_LSB_FIRST = 1
UNPACK_ENCODINGS = {"sign-magnitude": 0, "offset-binary": 1, "twos-complement": 2}


def unpack_table(bits, encoding="sign-magnitude", peak=48):
    """int8[2^bits]: the level of every code of a packed record in one of the three usual encodings ('sign-magnitude',
    'offset-binary', 'twos-complement', or the library's number), symmetric odd levels times peak // (2^bits - 1)
    (sgx_unpack_table; exact host code, needs no GPU)."""
    enc = UNPACK_ENCODINGS.get(encoding, encoding) if isinstance(encoding, str) else encoding
    if isinstance(enc, str):
        raise ValueError("the encoding of a packed record is one of %s, not %r" % (", ".join(sorted(UNPACK_ENCODINGS)), encoding))
    table = np.zeros(16, dtype=np.int8)
    check(lib().sgx_unpack_table(int(bits), int(enc), int(peak), _ptr(table)))
    return table[:1 << int(bits)].copy()


def unpack_tile():
    """Output bytes one workgroup of the unpacker makes: its tile seams lie at the multiples."""
    return _tile("sgx_unpack_tile")


DECIM_MAX_TAPS = 511
DECIM_MIN_FACTOR, DECIM_MAX_FACTOR = 2, 16
DECIM_OFFSET_BINARY = 1


def decim_design(fs, f0, bandwidth_hz, lanes, factor, n_taps=127, gain=0.0):
    """The band-pass of the decimation stage and where the band lands (sgx_decim_design; exact host code, needs no GPU):
    the band f0 +- bandwidth_hz / 2 of a record at rate fs - lanes 1: a real record, lanes 2: interleaved I/Q at the complex
    rate fs with f0 the offset from the centre - for decimation by `factor`.  gain <= 0: the gain that keeps a white
    input's rms.  Returns (taps, shift, info): taps int16[n_taps], or for lanes 2 int16[2 n_taps] with re and im
    interleaved; info = dict(fs_out, f_out, inverted)."""
    taps = np.zeros(2 * max(int(n_taps), 1), dtype=np.int16)
    shift, inv = C.c_int32(0), C.c_int32(0)
    fs_out, f_out = C.c_double(0), C.c_double(0)
    check(lib().sgx_decim_design(float(fs), float(f0), float(bandwidth_hz), int(lanes), int(factor), int(n_taps),
                                 float(gain), _ptr(taps), C.byref(shift), C.byref(fs_out), C.byref(f_out), C.byref(inv)))
    return taps[:int(lanes) * int(n_taps)].copy(), shift.value, dict(fs_out=fs_out.value, f_out=f_out.value,
                                                                   inverted=bool(inv.value))


def decim_tile():
    """Output bytes one workgroup of the decimator makes: its tile seams lie at the multiples."""
    return _tile("sgx_decim_tile")


RESAMP_MAX_TAPS = 1023
RESAMP_MAX_UP, RESAMP_MAX_DOWN = 16, 3
RESAMP_SHIFT = 14


def resamp_pair_ok(up, down):
    """Whether up / down is one of the 31 ratios the resampler takes: 1 <= down <= 3, down < up <= 16, coprime."""
    import math
    return 1 <= down <= RESAMP_MAX_DOWN and down < up <= RESAMP_MAX_UP and math.gcd(up, down) == 1


def resamp_design(fs, up, down=1, n_taps=0, cutoff_hz=0.0, gain=1.0):
    """The low-pass of the resampling stage (sgx_resamp_design; exact host code, needs no GPU): a Hann-windowed sinc at the
    stuffed rate fs up, cutoff cutoff_hz (0: half the lower of the two rates), n_taps taps (0: 24 up + 1).  Returns
    (taps int16[n_taps], shift, info); info = dict(fs_out)."""
    n = int(n_taps) if n_taps else 24 * int(up) + 1
    taps = np.zeros(max(n, 1), dtype=np.int16)
    shift, fs_out = C.c_int32(0), C.c_double(0)
    check(lib().sgx_resamp_design(float(fs), int(up), int(down), n, float(cutoff_hz), float(gain), _ptr(taps),
                                  C.byref(shift), C.byref(fs_out)))
    return taps[:n].copy(), shift.value, dict(fs_out=fs_out.value)


def resamp_tile():
    """Output bytes one workgroup of the resampler makes at up = 16; at another ratio its tile seams lie at the multiples
    of resamp_tile() * up // 16."""
    return _tile("sgx_resamp_tile")


ARRAY_MAX_ANTENNAS = 8
ARRAY_MAX_TAPS = 15
ARRAY_MAX_WEIGHTS = 64
ARRAY_SHIFT = 12
ARRAY_OFFSET_BINARY = 1
ARRAY_BLOCK_UNIT = 4096
ARRAY_MAX_BLOCKS = 1 << 20
ARRAY_MAX_WINDOW = 63


def array_design(rho, frames, lanes, ref=0, loading=1e-3, target_rms=12.0):
    """The power-inversion weights of the multi-antenna combiner (sgx_array_design; exact host code, needs no GPU) from the
    lag statistics rho, int64[A, A, K, lanes] of `frames` frames (Context.array_stats): the weights that minimise the output
    power while tap (K - 1) / 2 of antenna `ref` is held at 1, with `loading` x the mean diagonal added to the diagonal,
    scaled so that the output's rms per component is target_rms.  Returns (taps, shift, info): taps int16[A, K] - for
    lanes 2 int16[A, K, 2], re and im - and info = dict(weights float64[A, K] or complex128[A, K] before the gain, gain,
    suppression_db: the reference antenna's power over the output's before the gain)."""
    r = np.ascontiguousarray(rho, dtype=np.int64)
    la = int(lanes)
    if r.ndim != 4 or r.shape[0] != r.shape[1] or r.shape[3] != la:
        raise ValueError("rho has shape %r, expected (A, A, K, %d)" % (r.shape, la))
    A, K = r.shape[0], r.shape[2]
    taps = np.zeros((A, K, la), dtype=np.int16)
    w = np.zeros((A, K, la))
    shift, gain, supp = C.c_int32(0), C.c_double(0), C.c_double(0)
    check(lib().sgx_array_design(_ptr(r), int(frames), la, A, K, int(ref), float(loading), float(target_rms), _ptr(taps),
                                 C.byref(shift), _ptr(w), C.byref(gain), C.byref(supp)))
    weights = w[:, :, 0] + 1j * w[:, :, 1] if la == 2 else w[:, :, 0].copy()
    return (taps if la == 2 else taps[:, :, 0].copy()), shift.value, dict(weights=weights, gain=gain.value,
                                                                         suppression_db=supp.value)


def array_blocks(frames, block_frames):
    """The blocks of block_frames frames that `frames` frames make: the last one may be short."""
    return -(-int(frames) // int(block_frames)) if int(block_frames) > 0 else 0


def array_design_blocks(rho_blocks, frames, block_frames, window, lanes, ref=0, loading=1e-3, target_rms=12.0):
    """The power-inversion weights of every block of a record of `frames` frames (sgx_array_design_blocks; exact host code,
    needs no GPU) from its block statistics rho_blocks, int64[blocks, A, A, K, lanes] (Context.array_block_stats): block j
    is designed as array_design designs a record, from the summed statistics of the `window` blocks around it (odd,
    1 .. 63; fewer at the ends of the record).  A block whose window the design refuses as not positive definite - an
    all-zero stretch - holds the taps of the nearest designed block before it (a leading one: behind it).  Returns (taps,
    shift, info): taps int16[blocks, A, K] - for lanes 2 int16[blocks, A, K, 2] - and info = dict(weights float64 or
    complex128 [blocks, A, K] before the gain, gain and suppression_db float64[blocks], status uint8[blocks]: 1 for a
    block that holds another's taps)."""
    r = np.ascontiguousarray(rho_blocks, dtype=np.int64)
    la = int(lanes)
    if r.ndim != 5 or r.shape[1] != r.shape[2] or r.shape[4] != la:
        raise ValueError("rho_blocks has shape %r, expected (blocks, A, A, K, %d)" % (r.shape, la))
    nb, A, K = r.shape[0], r.shape[1], r.shape[3]
    taps = np.zeros((nb, A, K, la), dtype=np.int16)
    w = np.zeros((nb, A, K, la))
    gain, supp, status = np.zeros(nb), np.zeros(nb), np.zeros(nb, dtype=np.uint8)
    shift = C.c_int32(0)
    check(lib().sgx_array_design_blocks(_ptr(r), nb, int(frames), int(block_frames), int(window), la, A, K, int(ref),
                                        float(loading), float(target_rms), _ptr(taps), C.byref(shift), _ptr(w), _ptr(gain),
                                        _ptr(supp), _ptr(status)))
    weights = w[..., 0] + 1j * w[..., 1] if la == 2 else w[..., 0].copy()
    return (taps if la == 2 else taps[..., 0].copy()), shift.value, dict(weights=weights, gain=gain, suppression_db=supp,
                                                                        status=status)


def array_stats_tile():
    """Frames one workgroup of the array statistics kernel sums at a time: its tile seams lie at the multiples."""
    return _tile("sgx_array_stats_tile")


def combine_tile():
    """Output bytes one workgroup of the combiner makes: its tile seams lie at the multiples."""
    return _tile("sgx_combine_tile")


def _int16_taps(taps):
    a = np.asarray(taps)
    if a.dtype.kind not in "iu" or a.size and (a.min() < -32768 or a.max() > 32767):
        raise ValueError("taps must be integers that fit int16")
    return np.ascontiguousarray(a, dtype=np.int16).ravel()


def _rows(a):
    """(array, row stride in elements) of a 2-D float64 array whose rows are contiguous; copies anything else."""
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("expected a [channels, ms] array, got shape %r" % (a.shape,))
    if a.dtype != np.float64 or a.strides[1] != 8 or a.strides[0] % 8 or a.strides[0] < 8 * a.shape[1]:
        a = np.ascontiguousarray(a, dtype=np.float64)
    return a, (a.strides[0] // 8 if a.shape[0] > 1 else a.shape[1])


def device_count():
    n = C.c_int(0)
    rc = lib().sgx_device_count(C.byref(n))
    return n.value if rc == SGX_OK else 0


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _ms_done(ms_done, n):
    """(int32[n] array, its pointer argument) of a per-channel ms_done, or (None, None); the caller holds the array
    until its call has returned."""
    if ms_done is None:
        return None, None
    done = np.ascontiguousarray(ms_done, dtype=np.int32)
    if done.shape != (n,):
        raise ValueError("ms_done has shape %r, expected (%d,)" % (done.shape, n))
    return done, _ptr(done)


_ACQ_FIELDS = ("carrFreq", "codePhase", "peakMetric", "freqBin", "fineIdx")


def _acq_out(n):
    """(the five output arrays of a search over n PRNs, their pointers in the order every sgx_acquire* takes them)."""
    arrays = tuple(np.zeros(n, dtype=np.int32 if k in ("freqBin", "fineIdx") else np.float64) for k in _ACQ_FIELDS)
    return arrays, tuple(_ptr(a) for a in arrays)


def _acq_dict(arrays):
    return dict(zip(_ACQ_FIELDS, arrays))


def nav_bits(i_p_row, sub_frame_start):
    """uint8 bits (1 = positive 20-ms sum) of I_P[start-20 : start+30000], reference postNavigation.py:125-138."""
    a = np.ascontiguousarray(i_p_row, dtype=np.float64)
    out = np.zeros(1501, dtype=np.uint8)
    nb = C.c_int32(0)
    rc = lib().sgx_nav_bits(_ptr(a), a.shape[0], int(sub_frame_start), _ptr(out), C.byref(nb))
    if rc == SGX_E_RANGE:
        raise ValueError(last_error())
    check(rc)
    return out[:nb.value]


class Context(object):
    """One device context (hipStream + scratch) per GPU."""

    def __init__(self, settings, device=0, priority=0):
        """priority: stream priority class (-1 high, 0 normal, +1 low); contexts meant to run at the same time on
        one GPU take different classes (they then never share a hardware queue)."""
        self._h = _P()
        self._s = settings_struct(settings)
        check(lib().sgx_ctx_create_prio(C.byref(self._s), int(device), int(priority), C.byref(self._h)))
        self.device = int(device)
        self._records = weakref.WeakSet()   # live records of this context: freed (loader threads joined) before it
        self._token = 0                     # searches so far (search_token)

    def close(self):
        if self._h:
            for rec in list(self._records):
                rec.free()
            lib().sgx_ctx_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(lib().sgx_ctx_sync(self._h))

    def timing(self):
        t = Timing()
        check(lib().sgx_get_timing(self._h, C.byref(t)))
        return dict(acquire_ms=t.acquire_ms, acq_coarse_ms=t.acq_coarse_ms, acq_fine_ms=t.acq_fine_ms,
                    track_ms=t.track_ms, synth_ms=t.synth_ms, track_kernel=int(t.track_kernel),
                    track_members=int(t.track_members), track_streamed=int(t.track_streamed))

    def stream_rates(self, nbytes=1 << 30, reps=5):
        """(read GB/s, copy GB/s) measured on this device: the practical HBM roof next to the 8 TB/s datasheet peak."""
        r, w = C.c_double(0), C.c_double(0)
        check(lib().sgx_stream_rates(self._h, int(nbytes), int(reps), C.byref(r), C.byref(w)))
        return r.value, w.value

    def fft_forward(self, rows, nonzero_len=None):
        """The module-level fft_forward on this context's device."""
        return fft_forward(self._h, rows, nonzero_len)

    def fft_fused(self, mul_x, mul_f, rows, **kw):
        """The module-level fft_fused on this context's device."""
        return fft_fused(self._h, mul_x, mul_f, rows, **kw)

    # ---- records ----
    def upload(self, samples):
        """int8 samples - or, for a two-byte record, the file's bytes viewed as int8 (upload_bytes)."""
        a = np.ascontiguousarray(samples, dtype=np.int8)
        h = _P()
        check(lib().sgx_if_upload(self._h, _ptr(a), a.size, C.byref(h)))
        return Record(self, h, a.size)

    def upload_bytes(self, data):
        """The raw bytes of a record of any sample type (bytes / any contiguous array), as they lie in the file."""
        return self.upload(np.frombuffer(memoryview(np.ascontiguousarray(data)).cast('B'), dtype=np.int8))

    def upload_file(self, path, file_offset, n):
        """Stream bytes [file_offset, file_offset+n) of a raw int8 record file into HBM."""
        h = _P()
        check(lib().sgx_if_upload_file(self._h, os.fsencode(path), int(file_offset), int(n), C.byref(h)))
        ln = C.c_size_t(0)
        check(lib().sgx_if_length(h, C.byref(ln)))
        return Record(self, h, int(ln.value))

    def open_file(self, path, file_offset, n):
        """Like upload_file, but returns at once: the record fills in the background (file order) while
        acquisition and tracking already run on it.  Record.wait() blocks until everything is resident."""
        h = _P()
        check(lib().sgx_if_open_file(self._h, os.fsencode(path), int(file_offset), int(n), C.byref(h)))
        ln = C.c_size_t(0)
        check(lib().sgx_if_length(h, C.byref(ln)))
        return Record(self, h, int(ln.value))

    def synth(self, scene, n, offset=0):
        h = _P()
        sc = scene_struct(scene)
        check(lib().sgx_if_synth(self._h, C.byref(sc), int(offset), int(n), C.byref(h)))
        return Record(self, h, int(n))

    # ---- hot path ----
    def _search(self, fn, n, *args):
        """The search fn(ctx, *args, outputs of n PRNs ...) as the dict of its five output arrays; n None: a search that is
        only queued and has no outputs yet.  Any search takes the context's result page, so it supersedes a queued one that
        nobody has looked at: one search may be pending per context (PendingSearch)."""
        self._token += 1
        out, ptrs = _acq_out(n) if n is not None else ((), ())
        check(getattr(lib(), fn)(self._h, *args, *ptrs))
        return _acq_dict(out)

    @property
    def search_token(self):
        """Counts the searches on this context: a PendingSearch is the context's pending one while it still holds this."""
        return self._token

    def acquire(self, rec, offset, n_samples, prn0, n_blocks=2, noncoh=False):
        prn = np.ascontiguousarray(prn0, dtype=np.int32)
        return self._search("sgx_acquire", prn.size, rec._h, int(offset), int(n_samples), _ptr(prn), prn.size, int(n_blocks),
                            1 if noncoh else 0)

    def acquire_f64(self, signal, prn0, n_blocks=2, noncoh=False):
        """acquire() on a host signal of any real dtype (copied to HBM as fp64)."""
        sig = np.ascontiguousarray(signal, dtype=np.float64)
        prn = np.ascontiguousarray(prn0, dtype=np.int32)
        return self._search("sgx_acquire_f64", prn.size, _ptr(sig), sig.size, _ptr(prn), prn.size, int(n_blocks),
                            1 if noncoh else 0)

    def acquire_coherent(self, rec, offset, n_samples, prn0, coherent_ms=1, n_windows=2, noncoh=False, bin_step_hz=None):
        """acquire() with coherent_ms-ms windows (n_windows of them) on a bin_step_hz grid (None: 500 / coherent_ms)."""
        pa = acq_params(coherent_ms, n_windows, noncoh, bin_step_hz)
        prn = np.ascontiguousarray(prn0, dtype=np.int32)
        return self._search("sgx_acquire_coherent", prn.size, rec._h, int(offset), int(n_samples), _ptr(prn), prn.size,
                            C.byref(pa))

    def acquire_coherent_f64(self, signal, prn0, coherent_ms=1, n_windows=2, noncoh=False, bin_step_hz=None):
        """acquire_coherent() on a host signal of any real dtype (copied to HBM as fp64)."""
        pa = acq_params(coherent_ms, n_windows, noncoh, bin_step_hz)
        sig = np.ascontiguousarray(signal, dtype=np.float64)
        prn = np.ascontiguousarray(prn0, dtype=np.int32)
        return self._search("sgx_acquire_coherent_f64", prn.size, _ptr(sig), sig.size, _ptr(prn), prn.size, C.byref(pa))

    @staticmethod
    def acquire_coherent_plan(settings, coherent_ms=1, n_windows=2, noncoh=False, bin_step_hz=None):
        """The module-level acquire_coherent_plan (needs no device)."""
        return acquire_coherent_plan(settings, coherent_ms, n_windows, noncoh, bin_step_hz)

    def acquire_sharded(self, comm, rank, world, rec, offset, n_samples, n_prn_total=32, n_blocks=2, noncoh=False):
        """This rank's share of the PRN search + the peak gather as ONE library call (sgx_acquire_sharded): packed on the
        device, one ncclAllGather (comm: a Comm, or None for no collective), one look.  Returns the merged 32-entry arrays."""
        r = self._search("sgx_acquire_sharded", 32, comm._h if comm is not None else None, int(rank), int(world), rec._h,
                         int(offset), int(n_samples), int(n_prn_total), int(n_blocks), 1 if noncoh else 0)
        r["freqBin"], r["fineIdx"] = r["freqBin"].astype(np.int64), r["fineIdx"].astype(np.int64)
        return r

    # ---- the same without host round trips between the stages (include/sgx.h, "round 6") ----
    def acquire_begin(self, rec, offset, n_samples, prn0, n_blocks=2, noncoh=False):
        """Queue the search of acquire(); nothing is looked at.  acquire_end() returns what acquire() would have.  Returns
        the token of the queued search (PendingSearch) - only a search that was queued takes one."""
        prn = np.ascontiguousarray(prn0, dtype=np.int32)
        self._search("sgx_acquire_begin", None, rec._h, int(offset), int(n_samples), _ptr(prn), prn.size, int(n_blocks),
                     1 if noncoh else 0)
        return self._token

    def acquire_end(self, n):
        out, ptrs = _acq_out(n)
        check(lib().sgx_acquire_end(self._h, *ptrs))
        return _acq_dict(out)

    def track_chained(self, rec, n_ch, ms, rec_file_offset=0, data_type=DT_INT8):
        """preRun on the device behind the pending acquisition + the tracking kernel behind it, one wait.
        Returns None where the queued sequence does not apply (SGX_E_DEFER: run acquire_end, preRun and track instead),
        else (series[n_ch, 13, ms], ms_done[n_ch], PRN[n_ch], acquiredFreq[n_ch], codePhase[n_ch], n_active)."""
        out = pinned_empty((int(n_ch), NUM_SERIES, int(ms)))
        done = np.zeros(n_ch, dtype=np.int32)
        prn = np.zeros(n_ch, dtype=np.int32)
        freq = np.zeros(n_ch)
        cph = np.zeros(n_ch)
        n_act = C.c_int32(0)
        rc = lib().sgx_track_chained(self._h, rec._h, int(rec_file_offset), int(n_ch), int(ms), _ptr(out), _ptr(done),
                                     int(data_type), _ptr(prn), _ptr(freq), _ptr(cph), C.byref(n_act))
        if rc == SGX_E_DEFER:
            return None
        if rc == SGX_E_SILENT:     # (the table is complete too: the rows of .series are its first n_active channels)
            e = SilentChannelError(last_error(), out, done)
            e.table = (prn, freq, cph, n_act.value)
            raise e
        check(rc)
        return out, done, prn, freq, cph, n_act.value

    def probe_stats(self, rec, offset, n, fs_mhz):
        """(f, Pxx, hist, n_segments) of the record window: Welch PSD and histogram of Settings.probeData."""
        f = np.zeros(8193)
        pxx = np.zeros(8193)
        hist = np.zeros(255, dtype=np.int64)
        nseg = C.c_int32(0)
        rc = lib().sgx_probe_stats(self._h, rec._h, int(offset), int(n), float(fs_mhz), _ptr(f), _ptr(pxx),
                                   _ptr(hist), C.byref(nseg))
        if rc == SGX_E_RANGE:
            raise ValueError(last_error())
        check(rc)
        return f, pxx, hist, nseg.value

    def waterfall(self, rec, offset, n, fs_mhz, nperseg=16384, noverlap=1024, slice_len=None):
        """The record monitor (sgx_probe_waterfall): samples [offset, offset + n) of an int8 record cut into slices of
        slice_len samples (None: one slice), each slice's Welch spectrum - the density of probe_stats at segment length
        nperseg - and exact integer statistics.  Returns a Waterfall.  ValueError for what waterfall_plan refuses."""
        S = int(n) if slice_len is None else int(slice_len)
        ns = waterfall_plan(n, nperseg, noverlap, S)
        bins = int(nperseg) // 2 + 1
        f, pxx, hold = np.zeros(bins), np.zeros((ns, bins)), np.zeros(bins)
        moments, hist = np.zeros((ns, 4), dtype=np.int64), np.zeros((ns, 256), dtype=np.int64)
        nseg, got = np.zeros(ns, dtype=np.int64), C.c_int64(0)
        rc = lib().sgx_probe_waterfall(self._h, rec._h, int(offset), int(n), float(fs_mhz), int(nperseg), int(noverlap), S,
                                       _ptr(f), _ptr(pxx), _ptr(hold), _ptr(moments), _ptr(hist), _ptr(nseg), C.byref(got))
        if rc == SGX_E_RANGE:
            raise ValueError(last_error())
        check(rc)
        assert got.value == ns
        return Waterfall(f, pxx, hold, moments, hist, nseg, S)

    def waterfall_timing(self):
        """HIP-event time (ms) of the last waterfall()'s kernels."""
        t = C.c_float(0)
        check(lib().sgx_waterfall_timing(self._h, C.byref(t)))
        return t.value

    def find_preambles(self, i_p, search_start=0):
        """i_p: float64[n_ch, ms] -> int array firstSubFrame[n_ch] (0 = no verified preamble)."""
        a = np.ascontiguousarray(i_p, dtype=np.float64)
        out = np.zeros(a.shape[0], dtype=np.int32)
        rc = lib().sgx_find_preambles(self._h, _ptr(a), a.shape[0], a.shape[1], int(search_start), _ptr(out))
        if rc == SGX_E_RANGE:      # the exceptions the reference's numpy code raises on a record cut short
            msg = last_error()
            raise (IndexError if msg.startswith("IndexError") else ValueError)(msg)
        check(rc)
        return out.astype(int)

    def track_quality(self, i_p, q_p, params, ms_done=None):
        """C/N0 and lock detector of sgx_track_quality.  i_p, q_p: float64[n_ch, ms] - views with contiguous rows such as
        series[:, 3] and series[:, 7] of track() are passed as they lie; params: LockParams; ms_done: int[n_ch] or None.
        Returns (cno[n_ch, ms // W], carr_lock[n_ch, ms // W], pass bool[n_ch, ms // W], lost window int32[n_ch])."""
        a, sa = _rows(i_p)
        b, sb = _rows(q_p)
        if a.shape != b.shape:
            raise ValueError("I_P %r and Q_P %r differ in shape" % (a.shape, b.shape))
        if sa != sb:
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            sa = a.shape[1]
        n, ms = a.shape
        nw = ms // max(int(params.window), 1)
        cno = np.empty((n, nw))
        cl = np.empty((n, nw))
        ok = np.empty((n, nw), dtype=np.uint8)
        lost = np.empty(n, dtype=np.int32)
        done, done_p = _ms_done(ms_done, n)
        check(lib().sgx_track_quality(self._h, _ptr(a), _ptr(b), int(sa), int(n), int(ms),
                                      done_p, C.byref(params), _ptr(cno), _ptr(cl), _ptr(ok), _ptr(lost)))
        return cno, cl, ok.astype(bool), lost

    def track_replay(self, rec, chans, series, taps, ms_done=None, rec_file_offset=0, data_type=DT_INT8):
        """Multi-correlator replay of tracked channels (sgx_track_replay).  chans: (prn, acquiredFreq, codePhase) per
        channel as they were tracked, series: float64[n_ch, 13, ms] of track(), taps: code offsets in chips (1 .. 64 of
        them), ms_done: int[n_ch] or None.  Returns float64[n_ch, n_taps, 2, ms]: I then Q per tap."""
        n = len(chans)
        a = _series3(series, n)
        ms = a.shape[2]
        tp = np.ascontiguousarray(taps, dtype=np.float64).ravel()
        done, done_p = _ms_done(ms_done, n)
        out = np.zeros((n, tp.size, 2, ms))
        check(lib().sgx_track_replay(self._h, rec._h, int(rec_file_offset), C.cast(_chan_array(chans), _P), n, ms,
                                     done_p, _ptr(a), int(data_type), _ptr(tp), tp.size, _ptr(out)))
        return out

    def _timing(self, getter, n):
        """The n HIP-event times (ms) the library's sgx_*_timing `getter` reports for this context."""
        ms = [C.c_float(0) for _ in range(n)]
        check(getattr(lib(), getter)(self._h, *[C.byref(v) for v in ms]))
        return tuple(v.value for v in ms)

    def replay_timing(self):
        """(kernel ms, device ms) of the last track_replay on this context, from HIP events on its stream."""
        return self._timing("sgx_replay_timing", 2)

    def _stage(self, fn, args, n=None, counters=(), tail=()):
        """The new Record that the record stage fn(ctx, *args, &record, *tail, &counter ...) makes - of n bytes; None: as many
        as sgx_if_length says - with its int64 counters as the attributes named in `counters`."""
        h, cnt = _P(), [C.c_int64(0) for _ in counters]
        check(getattr(lib(), fn)(self._h, *args, C.byref(h), *tail, *[C.byref(v) for v in cnt]))
        if n is None:
            ln = C.c_size_t(0)
            check(lib().sgx_if_length(h, C.byref(ln)))
            n = int(ln.value)
        out = Record(self, h, n)
        for k, v in zip(counters, cnt):
            setattr(out, k, v.value)
        return out

    def filter_record(self, rec, taps, shift):
        """A new int8 record of the same length: `rec` through the zero-phase integer FIR of sgx_if_filter (taps: int16, an
        odd number of them up to 4095; y = clip((sum_k h[k] x[n + c - k] + 2^(shift-1)) >> shift, -127, 127))."""
        h16 = _int16_taps(taps)
        return self._stage("sgx_if_filter", (rec._h, _ptr(h16), h16.size, int(shift)), len(rec))

    def filter_timing(self):
        """Kernel ms of the last filter_record on this context, from HIP events on its stream."""
        return self._timing("sgx_filter_timing", 1)[0]

    def excise_record(self, rec, N=256, threshold=8.0, passes=3):
        """A new int8 record of the same length: `rec` cleared of swept interference (sgx_if_excise: segments of N samples at
        hop N / 2 under the root-Hann window, in each the bins above threshold x the mean of the kept bins zeroed, `passes`
        rounds, windowed overlap-add back).  Returns (record, info): segments, bins_cut, segments_cut, clipped and
        cut_per_segment (uint16 per segment)."""
        ok = EXCISE_MIN_SEGMENT <= int(N) <= EXCISE_MAX_SEGMENT      # (what is out of range is the library's to refuse)
        J = -(-len(rec) // (int(N) // 2)) + 1 if ok else 1
        per, info = np.zeros(J, dtype=np.uint16), ExciseInfo()
        out = self._stage("sgx_if_excise", (rec._h, int(N), float(threshold), int(passes)), len(rec),
                          tail=(C.byref(info), _ptr(per)))
        return out, _excise_info(info, per)

    def excise_timing(self):
        """Kernel ms of the last excise_record on this context, from HIP events on its stream."""
        return self._timing("sgx_excise_timing", 1)[0]

    def if_cancel(self, rec, chans, series, amp, ms_done=None, rec_file_offset=0, data_type=DT_INT8):
        """A new int8 record of the same length: `rec` with the tracked channels subtracted (sgx_if_cancel).  chans: (prn,
        acquiredFreq, codePhase) per channel as they were tracked, 1 .. 32 of them; series: float64[n_ch, 13, ms] of
        track(); amp: float64[n_ch, ms, 2] of cancel_design; ms_done: int[n_ch] or None.  The record's attribute `clipped`
        counts the outputs that lay outside [-127, 127] in front of the clip."""
        n = len(chans)
        ser = _series3(series, n)
        ms = ser.shape[2]
        am = _amp3(amp, n, ms)
        done, done_p = _ms_done(ms_done, n)
        return self._stage("sgx_if_cancel", (rec._h, int(rec_file_offset), C.cast(_chan_array(chans), _P), n, ms, done_p,
                                             _ptr(ser), int(data_type), _ptr(am)), len(rec), counters=("clipped",))

    def cancel_timing(self):
        """Kernel ms of the last if_cancel on this context, from HIP events on its stream."""
        return self._timing("sgx_cancel_timing", 1)[0]

    def iq_to_if(self, rec, taps, shift, q_first=False, offset_binary=False):
        """A new int8 record of the same length: `rec`, the raw bytes of an interleaved 8-bit I/Q file at complex rate fs_c,
        as the equivalent real record at 2 fs_c with IF = IF_bb + fs_c / 2 (sgx_if_from_iq: interpolation by 2 through the
        int16 taps, an odd number of them up to 255, a quarter-rate shift, the real part).  q_first: the file holds Q before
        I; offset_binary: its bytes are uint8 around 128."""
        h16 = _int16_taps(taps)
        flags = (IQ_Q_FIRST if q_first else 0) | (IQ_OFFSET_BINARY if offset_binary else 0)
        return self._stage("sgx_if_from_iq", (rec._h, _ptr(h16), h16.size, int(shift), flags), len(rec))

    def iq_timing(self):
        """Kernel ms of the last iq_to_if on this context, from HIP events on its stream."""
        return self._timing("sgx_iq_timing", 1)[0]

    def requant_stats(self, rec, dtype, offset=0, count=None):
        """Statistics of elements [offset, offset + count) (count None: to the end) of `rec`, the raw bytes of a file of
        int16 or float32 samples (sgx_requant_stats_of): dict(n_finite, n_nonfinite, max_abs, sum, sum_sq).  NaN and
        infinite samples are counted in n_nonfinite and left out of the rest; int16 sums are exact, float32 sums are
        taken in double in a fixed order (two calls agree bit for bit)."""
        dt, w = requant_type(dtype)
        if count is None:
            count = max(0, len(rec) // w - int(offset))
        st = RequantStats()
        check(lib().sgx_requant_stats_of(self._h, rec._h, dt, int(offset), int(count), C.byref(st)))
        return dict(n_finite=int(st.n_finite), n_nonfinite=int(st.n_nonfinite), max_abs=st.max_abs, sum=st.sum,
                    sum_sq=st.sum_sq)

    def requantize(self, rec, dtype, mult=1, shift=0, scale=1.0):
        """A new int8 record, one byte per element of `rec` (the raw bytes of a file of int16 or float32 samples), through
        one fixed gain (sgx_if_requantize).  int16: y = clip((x mult + 2^(shift-1)) >> shift, -127, 127); float32:
        y = clip(rint(x * float32(scale)), -127, 127), NaN -> 0.  The number of outputs on +-127 is left in the new
        record's `clipped`."""
        dt, w = requant_type(dtype)
        return self._stage("sgx_if_requantize", (rec._h, dt, int(mult), int(shift), float(scale)), len(rec) // w,
                           ("clipped",))

    def requant_timing(self):
        """(statistics kernel ms, quantiser kernel ms) of the last requant_stats and the last requantize on this context."""
        return self._timing("sgx_requant_timing", 2)

    def cond_stats(self, rec, dtype, lanes, block, blank_q4, offset_binary=False):
        """Per-block statistics of `rec`, the raw bytes of a file of int8, uint8 (offset binary) or int16 samples in
        frames of `lanes` elements and blocks of `block` frames (sgx_cond_block_stats): a COND_STATS_DTYPE array, one
        entry per block, every field an exact integer."""
        dt, w, flags = cond_type(dtype, offset_binary)
        cap = len(rec) // (w * max(int(lanes), 1) * max(int(block), 1)) + 1
        out = np.zeros(cap, dtype=COND_STATS_DTYPE)
        k = C.c_size_t(0)
        check(lib().sgx_cond_block_stats(self._h, rec._h, dt, int(lanes), int(block), int(blank_q4), flags, _ptr(out), cap,
                                         C.byref(k)))
        return out[:k.value]

    def condition(self, rec, dtype, lanes, block, plan, guard, offset_binary=False):
        """A new int8 record, one byte per element of `rec`: DC removed, scaled and blanked block by block as `plan` (a
        COND_PLAN_DTYPE array, one entry per block) says, hits dilated by `guard` frames (sgx_if_condition).  The blanked
        frames and the outputs on +-127 are left in the new record's `blanked` and `clipped`."""
        dt, w, flags = cond_type(dtype, offset_binary)
        p = np.ascontiguousarray(plan, dtype=COND_PLAN_DTYPE).ravel()
        return self._stage("sgx_if_condition", (rec._h, dt, int(lanes), int(block), flags, _ptr(p), p.size, int(guard)),
                           len(rec) // w, ("blanked", "clipped"))

    def cond_timing(self):
        """(statistics kernel ms, apply kernel ms) of the last cond_stats and the last condition on this context."""
        return self._timing("sgx_cond_timing", 2)

    def unpack(self, rec, bits, table, lsb_first=False, frame=1, first=0, take=1):
        """A new int8 record, one byte per selected field of `rec`, the raw bytes of a file of `bits`-bit samples (1, 2 or
        4) packed first field in the high bits (lsb_first: in the low bits), through `table` (2^bits int8 values, one per
        code; unpack_table makes the usual ones) (sgx_if_unpack).  Of every frame of `frame` fields (1, 2, 4, 8 or 16) the
        `take` fields from field `first` on are kept.  The exact count of each code among them is left in the new record's
        `code_counts` (int64[2^bits])."""
        b = int(bits)
        tab = np.zeros(16, dtype=np.int8)
        if b in (1, 2, 4):                         # (any other width is the library's to refuse)
            a = np.asarray(table)
            if a.ndim != 1 or a.size != 1 << b or a.dtype.kind not in "iu" or a.min() < -128 or a.max() > 127:
                raise ValueError("the table of a %d-bit record holds %d integers that fit int8" % (b, 1 << b))
            tab[:a.size] = a
        counts = np.zeros(16, dtype=np.int64)
        out = self._stage("sgx_if_unpack", (rec._h, b, UNPACK_LSB_FIRST if lsb_first else 0, int(frame), int(first), int(take),
                                            _ptr(tab)), tail=(_ptr(counts),))
        out.code_counts = counts[:1 << b].copy()
        return out

    def unpack_timing(self):
        """Kernel ms of the last unpack on this context, from HIP events on its stream."""
        return self._timing("sgx_unpack_timing", 1)[0]

    def decimate(self, rec, lanes, taps, shift, factor, offset_binary=False):
        """A new int8 record at 1 / factor of the rate: `rec` through the band-selecting integer FIR of sgx_if_decimate
        (factor 2 .. 16).  lanes 1: a real int8 record, taps int16[L]; lanes 2: interleaved I/Q, COMPLEX taps as
        int16[2 L], re and im interleaved.  L is odd, at most 511; decim_design makes the usual taps.  offset_binary: the
        input bytes are uint8 around 128.  Output frame m is the instant of input frame m factor.  The exact count of
        outputs whose value before the clip lay outside [-127, 127] is left in the new record's `clipped`."""
        h16 = _int16_taps(taps)
        la = int(lanes)
        if la == 2 and h16.size % 2:
            raise ValueError("the complex taps of an I/Q record are pairs (re, im): %d values are not" % h16.size)
        return self._stage("sgx_if_decimate", (rec._h, la, _ptr(h16), h16.size // 2 if la == 2 else h16.size, int(shift),
                                               int(factor), DECIM_OFFSET_BINARY if offset_binary else 0), counters=("clipped",))

    def decim_timing(self):
        """Kernel ms of the last decimate on this context, from HIP events on its stream."""
        return self._timing("sgx_decim_timing", 1)[0]

    def resample(self, rec, taps, shift, up, down=1):
        """A new int8 record at up / down of the rate: the real int8 record `rec` through the polyphase integer FIR of
        sgx_if_resample (1 <= down <= 3, down < up <= 16, coprime).  taps int16[Lh], Lh odd, at most 1023, at the stuffed
        rate; resamp_design makes the usual ones.  Output sample m is the instant of input position m down / up.  The
        exact count of outputs whose value before the clip lay outside [-127, 127] is left in the new record's `clipped`."""
        h16 = _int16_taps(taps)
        return self._stage("sgx_if_resample", (rec._h, _ptr(h16), h16.size, int(shift), int(up), int(down)),
                           counters=("clipped",))

    def resamp_timing(self):
        """Kernel ms of the last resample on this context, from HIP events on its stream."""
        return self._timing("sgx_resamp_timing", 1)[0]

    def array_stats(self, rec, lanes, A, K, offset_binary=False):
        """The exact lag statistics of `rec`, an int8 record of frames of A antennas (byte (f A + a) lanes + l: component l
        of antenna a at frame f; lanes 2: interleaved I/Q), as int64[A, A, K, lanes] (sgx_array_stats):
        rho[a, b, d] = sum_f x_a[f + d] conj(x_b[f]), real part then imaginary part.  K odd, 1 .. 15, A 2 .. 8, A K <= 64.
        offset_binary: the input bytes are uint8 around 128."""
        rho = np.zeros((max(int(A), 0), max(int(A), 0), max(int(K), 0), 2 if int(lanes) == 2 else 1), dtype=np.int64)
        buf = np.zeros(max(rho.size, 1), dtype=np.int64)
        check(lib().sgx_array_stats(self._h, rec._h, int(lanes), int(A), int(K), ARRAY_OFFSET_BINARY if offset_binary else 0,
                                    _ptr(buf)))
        rho[...] = buf[:rho.size].reshape(rho.shape)
        return rho

    def array_stats_timing(self):
        """Kernel ms of the last array_stats on this context, from HIP events on its stream."""
        return self._timing("sgx_array_stats_timing", 1)[0]

    def combine(self, rec, lanes, A, taps, shift, offset_binary=False):
        """A new int8 record of one frame per frame of `rec` (frames of A antennas, as array_stats reads them): every antenna
        through its own integer FIR and all of them summed (sgx_if_combine).  taps int16[A, K], for lanes 2 COMPLEX as
        int16[A, K, 2]; K odd, at most 15; array_design makes the usual ones.  Output frame f is the instant of input frame
        f.  The exact count of outputs whose value before the clip lay outside [-127, 127] is left in the new record's
        `clipped`."""
        a = np.asarray(taps)
        la, n_a = int(lanes), int(A)
        h16 = _int16_taps(a)
        per = n_a * la
        if per <= 0 or h16.size % per:
            raise ValueError("the taps of %d antennas (lanes %d) are %d values per tap, %d values are not" % (n_a, la, per, h16.size))
        return self._stage("sgx_if_combine", (rec._h, la, n_a, _ptr(h16), h16.size // per, int(shift),
                                              ARRAY_OFFSET_BINARY if offset_binary else 0), counters=("clipped",))

    def combine_timing(self):
        """Kernel ms of the last combine on this context, from HIP events on its stream."""
        return self._timing("sgx_combine_timing", 1)[0]

    def array_block_stats(self, rec, lanes, A, K, block_frames, offset_binary=False):
        """The exact lag statistics of `rec` as array_stats takes them, block by block (sgx_array_block_stats):
        int64[blocks, A, A, K, lanes], block j holding the terms whose x_b frame lies in [j block_frames, (j + 1)
        block_frames) - the x_a frame may lie in the next block.  block_frames is a multiple of ARRAY_BLOCK_UNIT; the sum
        over the blocks is array_stats' result."""
        la, n_a, k = (2 if int(lanes) == 2 else 1), max(int(A), 0), max(int(K), 0)
        frames = len(rec) // (n_a * la) if n_a else 0
        rho = np.zeros((array_blocks(frames, block_frames), n_a, n_a, k, la), dtype=np.int64)
        buf = rho.reshape(-1) if rho.size else np.zeros(1, dtype=np.int64)
        check(lib().sgx_array_block_stats(self._h, rec._h, int(lanes), int(A), int(K),
                                          ARRAY_OFFSET_BINARY if offset_binary else 0, int(block_frames), _ptr(buf)))
        return rho

    def array_block_stats_timing(self):
        """Kernel ms of the last array_block_stats on this context, from HIP events on its stream."""
        return self._timing("sgx_array_block_stats_timing", 1)[0]

    def combine_blocks(self, rec, lanes, A, taps, block_frames, shift, offset_binary=False):
        """combine() with a set of taps per block of block_frames frames (sgx_if_combine_blocks): OUTPUT frame f is made with
        set f // block_frames, from input frames that may lie in the neighbouring block.  taps int16[blocks, A, K], for
        lanes 2 int16[blocks, A, K, 2]; array_design_blocks makes the usual ones.  The exact count of outputs whose value
        before the clip lay outside [-127, 127] is left in the new record's `clipped`."""
        a = np.asarray(taps)
        la, n_a = int(lanes), int(A)
        if a.ndim != (4 if la == 2 else 3) or a.shape[1] != n_a or (la == 2 and a.shape[3] != 2):
            raise ValueError("the taps of the blocks have shape %r, expected (blocks, %d, K%s)"
                             % (a.shape, n_a, ", 2" if la == 2 else ""))
        h16 = _int16_taps(a)
        if not h16.size:
            h16 = np.zeros(1, dtype=np.int16)
        return self._stage("sgx_if_combine_blocks", (rec._h, la, n_a, _ptr(h16), a.shape[0], int(block_frames), a.shape[2],
                                                     int(shift), ARRAY_OFFSET_BINARY if offset_binary else 0),
                           counters=("clipped",))

    def combine_blocks_timing(self):
        """Kernel ms of the last combine_blocks on this context, from HIP events on its stream."""
        return self._timing("sgx_combine_blocks_timing", 1)[0]

    def track(self, rec, chans, ms, rec_file_offset=0, data_type=DT_INT8):
        """chans: sequence of (prn, acquiredFreq, codePhase). Returns (series[n_ch,13,ms], ms_done).
        SilentChannelError (a ValueError, as in the reference) where a channel met a block of exactly zero sums.
        data_type DT_INT16: `rec` holds the BYTES of a little-endian int16 file (see sgx_track_ex in include/sgx.h)."""
        n = len(chans)
        arr = (ChanInit * n)()
        for i, (prn, f, cp) in enumerate(chans):
            arr[i] = ChanInit(float(f), float(cp), int(prn), 0)
        out = pinned_empty((n, NUM_SERIES, int(ms)))
        done = np.zeros(n, dtype=np.int32)
        rc = lib().sgx_track_ex(self._h, rec._h, int(rec_file_offset), C.cast(arr, _P), n, int(ms), _ptr(out),
                                _ptr(done), int(data_type))
        if rc == SGX_E_SILENT:     # a channel went silent: the reference's ValueError, with what was tracked until then
            raise SilentChannelError(last_error(), out, done)
        check(rc)
        return out, done

    def track_coherent(self, rec, chans, ms, params, bit_edge=None, rec_file_offset=0, data_type=DT_INT8):
        """sgx_track_coherent: bit-aligned coherent tracking of an int8 record.  chans: sequence of (prn, acquiredFreq,
        codePhase); params: CohParams (coh_params); bit_edge: per channel -1 (find it, the default) or 0 .. 19.
        Returns (series[n_ch,13,ms], ms_done, bit_edge, coh_start, edge_energy[n_ch,20]); SilentChannelError as track(),
        the three further arrays attached to it as .bit_edge, .coh_start and .edge_energy."""
        if int(data_type) != DT_INT8:
            raise TypeError("coherent tracking reads int8 records: condition or requantise other sample types first "
                            "(data_type %d)" % int(data_type))
        n = len(chans)
        arr = (ChanInit * n)()
        for i, (prn, f, cp) in enumerate(chans):
            arr[i] = ChanInit(float(f), float(cp), int(prn), 0)
        edge_in = np.full(n, -1, dtype=np.int32) if bit_edge is None else np.ascontiguousarray(bit_edge, dtype=np.int32)
        if edge_in.shape != (n,):
            raise ValueError("bit_edge holds one value per channel")
        out = pinned_empty((n, NUM_SERIES, int(ms)))
        done, edge, start = (np.zeros(n, dtype=np.int32) for _ in range(3))
        energy = np.zeros((n, 20))
        rc = lib().sgx_track_coherent(self._h, rec._h, int(rec_file_offset), C.cast(arr, _P), n, int(ms), C.byref(params),
                                      _ptr(edge_in), _ptr(out), _ptr(done), _ptr(edge), _ptr(start), _ptr(energy))
        if rc == SGX_E_SILENT:
            e = SilentChannelError(last_error(), out, done)
            e.bit_edge, e.coh_start, e.edge_energy = edge, start, energy
            raise e
        check(rc)
        return out, done, edge, start, energy


class Record(object):
    """int8 IF record resident in HBM."""

    def __init__(self, ctx, handle, n):
        self.ctx = ctx
        self._h = handle
        self.n = n
        ctx._records.add(self)

    def __len__(self):
        return self.n

    def wait(self, n=0):
        """Block until the first n samples (0 = all) of a record opened with Context.open_file are resident."""
        check(lib().sgx_if_wait(self.ctx._h, self._h, int(n)))

    def download(self, offset=0, n=None):
        n = self.n - offset if n is None else n
        out = np.empty(n, dtype=np.int8)
        check(lib().sgx_if_download(self.ctx._h, self._h, int(offset), int(n), _ptr(out)))
        return out

    def free(self):
        if self._h:
            # (a context that is already gone: sgx_if_free(NULL, h) still joins the loader thread and frees the HBM)
            lib().sgx_if_free(self.ctx._h if self.ctx._h else None, self._h)
        self._h = _P()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Comm(object):
    """RCCL communicator for the acquisition peak gather (one process per GPU)."""

    def __init__(self, ctx, n_ranks, rank, unique_id):
        self._h = _P()
        self.n_ranks = n_ranks
        uid = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        check(lib().sgx_comm_create(ctx._h, n_ranks, rank, C.cast(uid, _P), C.byref(self._h)))

    @staticmethod
    def unique_id():
        uid = (C.c_uint8 * 128)()
        check(lib().sgx_comm_unique_id(C.cast(uid, _P)))
        return bytes(uid)

    def allgather(self, payload):
        send = np.ascontiguousarray(payload).view(np.uint8).ravel()
        recv = np.empty(send.size * self.n_ranks, dtype=np.uint8)
        check(lib().sgx_comm_allgather(self._h, _ptr(send), _ptr(recv), send.size))
        return recv.reshape(self.n_ranks, send.size)

    def close(self):
        if self._h:
            lib().sgx_comm_destroy(self._h)
            self._h = _P()
