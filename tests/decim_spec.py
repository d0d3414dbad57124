"""numpy restatement of the decimation stage (include/sgx.h: sgx_decim_design, sgx_if_decimate): the contract the host
design code and the HIP kernel (csrc/sgx_decim.hip) are tested against.  Integers (int64) only where samples are touched:
any summation order gives the same bytes.  Test infrastructure, not product code."""
import numpy as np

MAX_TAPS = 511
MAX_TAP = 32512          # 127 * 256: every tap component splits into two signed bytes, h = 256 hi + lo
DESIGN_SHIFT = 14
OFFSET_BINARY = 1
MIN_FACTOR, MAX_FACTOR = 2, 16
DEFAULT_TAPS = 127       # Settings.decimTaps
DEFAULT_BANDWIDTH = 2.046e6


def check(h, S, lanes, D, flags=0, n_bytes=0):
    """The preconditions of decimate(); the library refuses what fails them with SGX_E_ARG.  h: int16[L] for lanes 1,
    int16[2 L] (re, im interleaved) for lanes 2."""
    if int(lanes) not in (1, 2):
        raise ValueError("lanes must be 1 or 2")
    if not (MIN_FACTOR <= int(D) <= MAX_FACTOR):
        raise ValueError("D must be %d .. %d" % (MIN_FACTOR, MAX_FACTOR))
    h = np.asarray(h)
    if h.size % int(lanes):
        raise ValueError("complex taps are pairs")
    L = h.size // int(lanes)
    if not (1 <= L <= MAX_TAPS and L % 2 == 1):
        raise ValueError("n_taps must be odd, 1 .. %d" % MAX_TAPS)
    if not (0 <= int(S) <= 30):
        raise ValueError("shift must be 0 .. 30")
    a = np.abs(h.astype(np.int64))
    if a.max() > MAX_TAP:
        raise ValueError("a tap component must be <= %d in magnitude" % MAX_TAP)
    if 128 * int(a.sum()) >= 2 ** 31:
        raise ValueError("128 sum|h| must be < 2^31 (lanes 2: the sum of |re| + |im|)")
    if int(flags) & ~OFFSET_BINARY:
        raise ValueError("unknown flag bits")
    if int(lanes) == 2 and int(n_bytes) % 2:
        raise ValueError("an I/Q record holds whole pairs: N must be even")


def samples(b, flags=0):
    """The record's bytes as int64 (any 8-bit dtype: only the bit patterns count)."""
    x = np.ascontiguousarray(b).view(np.uint8)
    if int(flags) & OFFSET_BINARY:
        x = x ^ np.uint8(0x80)               # byte - 128, read as int8
    return x.view(np.int8).astype(np.int64)


def fir_direct(x, h, D, n_out):
    """sum_k h[k] x[m D + c - k] for m < n_out, x = 0 outside; int64.  The contract as it is written, tap by tap."""
    L = h.size
    c = (L - 1) // 2
    pad = np.zeros(c + n_out * D + c + 1, dtype=np.int64)
    pad[c:c + x.size] = x                    # pad[c + n] = x[n]
    acc = np.zeros(n_out, dtype=np.int64)
    for k in range(L):                       # x[m D + c - k] = pad[m D + 2 c - k]
        if h[k]:
            acc += int(h[k]) * pad[2 * c - k:2 * c - k + n_out * D:D][:n_out]
    return acc


def _fir_at(x, h, D, n_out):
    """fir_direct phase by phase - the same int64 sums in another order, several times faster on the long records of the
    scenes: with k = c - q D - p, y[m] = sum_p sum_q h[c - q D - p] x[(m + q) D + p]."""
    L = h.size
    c = (L - 1) // 2
    acc = np.zeros(n_out, dtype=np.int64)
    if n_out == 0:
        return acc
    for p in range(D):
        q_min, q_max = -((c + p) // D), (c - p) // D          # the q with 0 <= c - q D - p < L
        if q_max < q_min:
            continue
        g = h[c - np.arange(q_min, q_max + 1) * D - p]
        plane = x[p::D]
        ext = np.zeros(n_out + q_max - q_min, dtype=np.int64)   # ext[i] = plane[i + q_min], 0 outside
        lo = max(0, q_min)
        hi = min(plane.size, ext.size + q_min)
        if hi > lo:
            ext[lo - q_min:hi - q_min] = plane[lo:hi]
        acc += np.correlate(ext, g, mode="valid")
    return acc


def sums(b, h, lanes, D, flags=0):
    """The sums in front of the rounding, int64: [n_out] for lanes 1, [n_out, 2] (Re w, Im w) for lanes 2."""
    x = samples(b, flags)
    h = np.asarray(h).astype(np.int64)
    if int(lanes) == 1:
        return _fir_at(x, h, D, -(-x.size // D))
    I, Q = x[0::2], x[1::2]
    hr, hi = h[0::2], h[1::2]
    n_out = -(-I.size // D)
    re = _fir_at(I, hr, D, n_out) - _fir_at(Q, hi, D, n_out)
    im = _fir_at(Q, hr, D, n_out) + _fir_at(I, hi, D, n_out)
    return np.stack([re, im], axis=1)


def quantise(a, S):
    """(int8 bytes, mask of the clipped ones) of sums a: q(a) = clip((a + (S ? 2^(S-1) : 0)) >> S, -127, 127), and whether
    the value in front of the clip lay outside [-127, 127]."""
    a = np.asarray(a, dtype=np.int64).reshape(-1)
    assert a.size == 0 or np.abs(a).max() < 2 ** 31
    S = int(S)
    if S:
        a = (a + (1 << (S - 1))) >> S        # arithmetic shift: floor
    return np.clip(a, -127, 127).astype(np.int8), (a < -127) | (a > 127)


def decimate(b, h, S, lanes, D, flags=0):
    """(int8 output bytes, clipped).  lanes 1: y[m] = q(sum_k h[k] x[m D + c - k]), m < ceil(N / D).  lanes 2:
    z[n] = b[2n] + j b[2n+1], w[m] = sum_k h[k] z[m D + c - k] with complex h, bytes q(Re w[m]), q(Im w[m]),
    m < ceil(N/2 / D).  q as quantise(); clipped counts the output bytes whose value in front of the clip lay outside
    [-127, 127]."""
    b = np.ascontiguousarray(b)
    h = np.asarray(h)
    assert b.dtype.itemsize == 1 and h.dtype == np.int16
    check(h, S, lanes, D, flags, b.size)
    y, over = quantise(sums(b, h, lanes, D, flags), S)
    return y, int(np.count_nonzero(over))


def default_gain(fs, bandwidth, lanes):
    return float(np.sqrt((float(fs) / (2.0 if int(lanes) == 1 else 1.0)) / float(bandwidth)))


def output_settings(fs, f0, bandwidth, lanes, D):
    """(fs_out, f_out, inverted) of the decimated record; ValueError where the band would alias onto itself."""
    fs, f0, bandwidth, D = float(fs), float(f0), float(bandwidth), int(D)
    if not (np.isfinite(fs) and fs > 0 and np.isfinite(bandwidth) and bandwidth > 0 and np.isfinite(f0)):
        raise ValueError("fs and bandwidth must be finite and positive, f0 finite")
    if int(lanes) not in (1, 2) or not (MIN_FACTOR <= D <= MAX_FACTOR):
        raise ValueError("lanes must be 1 or 2, D %d .. %d" % (MIN_FACTOR, MAX_FACTOR))
    fo = fs / float(D)
    half = fo / 2.0
    if int(lanes) == 2:
        if not bandwidth < fo:
            raise ValueError("bandwidth >= fs / D")
        return fo, (f0 + half) % fo - half, False       # (Python's float %: fmod brought to the divisor's sign)
    z = float(np.floor(f0 / half))
    lo, hi = f0 - bandwidth / 2.0, f0 + bandwidth / 2.0
    if not (0 <= z < D and lo > z * half and hi < (z + 1.0) * half):
        raise ValueError("the band does not lie strictly inside one Nyquist zone of fs / D")
    inverted = bool(int(z) & 1)
    return fo, ((z + 1.0) * half - f0) if inverted else (f0 - z * half), inverted


def design_unrounded(fs, f0, bandwidth, lanes, D, L, gain=0.0):
    """The taps in front of the rounding, float64[L] (lanes 1) or float64[2 L] (re, im interleaved): with m = k - c
    2^14 g (bandwidth / fs) sinc(bandwidth m / fs) hann_L[k] times 2 cos(2 pi f0 m / fs) or e^{j 2 pi f0 m / fs}."""
    output_settings(fs, f0, bandwidth, lanes, D)
    fs, f0, bandwidth, L, gain = float(fs), float(f0), float(bandwidth), int(L), float(gain)
    if not (1 <= L <= MAX_TAPS and L % 2 == 1):
        raise ValueError("n_taps must be odd, 1 .. %d" % MAX_TAPS)
    if not np.isfinite(gain):
        raise ValueError("gain must be finite")
    g = gain if gain > 0 else default_gain(fs, bandwidth, lanes)
    c = (L - 1) // 2
    k = np.arange(L, dtype=np.float64)
    m = k - c
    t = bandwidth * m / fs
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.sin(np.pi * t) / (np.pi * t)
    sinc[c] = 1.0
    win = np.ones(L) if L == 1 else 0.5 - 0.5 * np.cos(2.0 * np.pi * k / float(L - 1))
    lp = (bandwidth / fs) * sinc * win
    ph = 2.0 * np.pi * f0 * m / fs
    a = float(1 << DESIGN_SHIFT) * g * lp
    if int(lanes) == 1:
        return a * (2.0 * np.cos(ph))
    u = np.empty(2 * L)
    u[0::2] = a * np.cos(ph)
    u[1::2] = a * np.sin(ph)
    return u


def design(fs, f0, bandwidth, lanes, D, L, gain=0.0):
    """(int16 taps, shift, fs_out, f_out, inverted): design_unrounded rounded half to even; ValueError for a tap that
    decimate() does not take."""
    u = np.rint(design_unrounded(fs, f0, bandwidth, lanes, D, L, gain))
    if np.abs(u).max() > MAX_TAP or 128 * int(np.abs(u).sum()) >= 2 ** 31:
        raise ValueError("a tap leaves what the decimator takes")
    return (u.astype(np.int16), DESIGN_SHIFT) + output_settings(fs, f0, bandwidth, lanes, D)


def rounding_margin(fs, f0, bandwidth, lanes, D, L, gain=0.0):
    """Smallest distance of an unrounded tap from a rounding boundary (k + 1/2)."""
    u = design_unrounded(fs, f0, bandwidth, lanes, D, L, gain)
    return float(np.min(np.abs((u - np.floor(u)) - 0.5)))
