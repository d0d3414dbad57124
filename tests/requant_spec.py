"""numpy restatement of the requantiser in front of the I/Q converter (include/sgx.h: sgx_requant_stats_of,
sgx_requant_gain, sgx_if_requantize): the contract the host gain code and the HIP kernels (csrc/sgx_requant.hip) are tested
against.  A record of N bytes holds n = N / w little-endian int16 (w = 2) or IEEE float32 (w = 4) elements; I and Q share
one gain, so every step is elementwise and knows nothing of pairs.  Test infrastructure, not product code."""
import math

import numpy as np

INT16 = np.dtype("<i2")
FLOAT32 = np.dtype("<f4")
MAX_MULT = 32767
MAX_SHIFT = 30
SCALE_MIN = 2.0 ** -100
SCALE_MAX = 2.0 ** 100
DEFAULT_TARGET_RMS = 12.0    # Settings.iqTargetRms: the noise level of the scenes of tests/iq_cases.py


def width(dtype):
    dt = np.dtype(dtype)
    if dt not in (INT16, FLOAT32):
        raise ValueError("data_type must be int16 or float32")
    return dt.itemsize


def elements(b, dtype):
    """The record's bytes (any array, only its bytes count) as its elements."""
    w = width(dtype)
    raw = np.ascontiguousarray(b).view(np.uint8).ravel()
    if raw.size % w:
        raise ValueError("a record of %d bytes does not hold whole %d-byte elements" % (raw.size, w))
    return raw.view(INT16 if w == 2 else FLOAT32)


def check_window(n, offset, count):
    if offset < 0 or count < 0 or offset > n or count > n - offset:
        raise ValueError("window [%d, %d) outside the %d elements of the record" % (offset, offset + count, n))


def check_gain(dtype, mult=1, shift=0, scale=1.0):
    """The preconditions of quantise(); the library refuses what fails them with SGX_E_ARG."""
    if width(dtype) == 2:
        if not 1 <= int(mult) <= MAX_MULT:
            raise ValueError("mult must be 1 .. %d" % MAX_MULT)
        if not 0 <= int(shift) <= MAX_SHIFT:
            raise ValueError("shift must be 0 .. %d" % MAX_SHIFT)
    elif not (math.isfinite(scale) and SCALE_MIN <= scale <= SCALE_MAX):
        raise ValueError("scale must lie in [2^-100, 2^100]")


def stats(b, dtype, offset=0, count=None):
    """Statistics of elements [offset, offset + count): dict(n_finite, n_nonfinite, max_abs, sum, sum_sq, sum_abs).
    int16: the sums are exact integers, converted to double once (float(int)).  float32: NaN and +-inf are counted in
    n_nonfinite and left out of everything else; sum and sum_sq are the CORRECTLY ROUNDED sums (math.fsum) of the elements
    and of their squares in double (a float32 squared is exact in double); the library sums in a fixed order and may differ
    from them by bounds(); sum_abs (fsum of |x|) is what the bound of `sum` needs."""
    x = elements(b, dtype)
    count = x.size - offset if count is None else count
    check_window(x.size, offset, count)
    x = x[offset:offset + count]
    if x.dtype == INT16:
        v = x.astype(np.int64)
        s, q = int(v.sum()), int((v * v).sum())          # (|sum_sq| <= 2^30 count: exact in int64 below 2^33 elements)
        return dict(n_finite=int(count), n_nonfinite=0, max_abs=float(np.abs(v).max()) if count else 0.0,
                    sum=float(s), sum_sq=float(q), sum_abs=float(int(np.abs(v).sum())))
    ok = np.isfinite(x)
    d = x[ok].astype(np.float64)
    return dict(n_finite=int(d.size), n_nonfinite=int(count - d.size), max_abs=float(np.abs(d).max()) if d.size else 0.0,
                sum=math.fsum(d), sum_sq=math.fsum(d * d), sum_abs=math.fsum(np.abs(d)))


def bounds(st, count):
    """(bound of |sum - fsum|, bound of |sum_sq - fsum|) of a float32 window of `count` elements: the worst case of
    recursive summation of `count` doubles in ANY order, count * 2^-52 times the sum of the magnitudes."""
    return count * 2.0 ** -52 * st["sum_abs"], count * 2.0 ** -52 * st["sum_sq"]


def gain(n_finite, sum_sq, target_rms=DEFAULT_TARGET_RMS):
    """(mult, shift, scale) of a record with these statistics: exact host arithmetic.
    rms = sqrt(sum_sq / n_finite), g = target_rms / rms (g = 1 for n_finite = 0 or an rms that is not > 0).
    int16: shift = the largest S in 0 .. 30 with rint(g 2^S) <= 32767 (half to even), mult = max(1, rint(g 2^S)); if even
    S = 0 gives more: mult = 32767, shift = 0.  float32: scale = float32(g) clamped to [2^-100, 2^100]."""
    if not (0.0 < target_rms <= 127.0):
        raise ValueError("target_rms must lie in (0, 127]")
    g = 1.0
    if n_finite > 0:
        with np.errstate(all="ignore"):
            rms = np.sqrt(np.float64(sum_sq) / np.float64(n_finite))
            if rms > 0.0:
                g = float(np.float64(target_rms) / rms)
    mult, shift = MAX_MULT, 0
    for S in range(MAX_SHIFT, -1, -1):
        r = np.rint(math.ldexp(g, S))                    # (ldexp: exact)
        if r <= MAX_MULT:
            mult, shift = max(1, int(r)), S
            break
    with np.errstate(all="ignore"):
        gf = np.float32(g)
    gf = np.float32(min(max(float(gf), SCALE_MIN), SCALE_MAX))
    return mult, shift, gf


def quantise(b, dtype, mult=1, shift=0, scale=1.0):
    """n int8 bytes, element i of the record -> byte i.
    int16:   y = clip((x mult + ((1 << shift) >> 1)) >> shift, -127, 127), floor shift; |x mult| + 2^(shift-1) < 2^31.
    float32: y = clip(rint(x *f32 scale), -127, 127): one float32 multiply, round to nearest even; NaN -> 0, +-inf ->
             +-127.  With scale <= 2^100 a denormal x (or product) rounds to 0 whether or not denormals are flushed."""
    check_gain(dtype, mult, shift, scale)
    x = elements(b, dtype)
    if x.dtype == INT16:
        a = x.astype(np.int64) * int(mult) + ((1 << int(shift)) >> 1)
        assert x.size == 0 or np.abs(a).max() < 2 ** 31
        return np.clip(a >> int(shift), -127, 127).astype(np.int8)
    with np.errstate(all="ignore"):
        p = x.astype(np.float32) * np.float32(scale)
        assert p.dtype == np.float32
        r = np.clip(np.rint(p), -127.0, 127.0)
    return np.where(np.isnan(p), np.float32(0.0), r).astype(np.int8)


def clipped_share(y):
    """Share of the output samples on +-127."""
    y = np.asarray(y)
    return float(np.count_nonzero(np.abs(y.astype(np.int16)) == 127)) / y.size if y.size else 0.0
