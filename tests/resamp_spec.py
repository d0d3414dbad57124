"""numpy restatement of the resampling stage (include/sgx.h: sgx_resamp_design, sgx_if_resample): the contract the host
design code and the HIP kernel (csrc/sgx_resamp.hip) are tested against.  Integers (int64) only where samples are touched:
any summation order gives the same bytes.  Test infrastructure, not product code."""
from math import gcd

import numpy as np

MAX_TAPS = 1023
MAX_TAP = 32512          # 127 * 256: every tap splits into two signed bytes, h = 256 hi + lo
DESIGN_SHIFT = 14
MAX_UP, MAX_DOWN = 16, 3
PAIRS = tuple((L, M) for M in range(1, MAX_DOWN + 1) for L in range(M + 1, MAX_UP + 1) if gcd(L, M) == 1)
assert len(PAIRS) == 31


def default_taps(L):
    """Settings.resampTaps = 0: 24 taps per phase and the centre."""
    return 24 * int(L) + 1


def check(h, S, L, M):
    """The preconditions of resample(); the library refuses what fails them with SGX_E_ARG."""
    if (int(L), int(M)) not in PAIRS:
        raise ValueError("L / M must be one of the 31 pairs: 1 <= M <= 3, M < L <= 16, gcd(L, M) = 1")
    h = np.asarray(h)
    if not (1 <= h.size <= MAX_TAPS and h.size % 2 == 1):
        raise ValueError("n_taps must be odd, 1 .. %d" % MAX_TAPS)
    if not (0 <= int(S) <= 30):
        raise ValueError("shift must be 0 .. 30")
    a = np.abs(h.astype(np.int64))
    if a.max() > MAX_TAP:
        raise ValueError("a tap must be <= %d in magnitude" % MAX_TAP)
    if 128 * int(a.sum()) >= 2 ** 31:
        raise ValueError("128 sum|h| must be < 2^31")


def samples(b):
    """The record's bytes as int64 (any 8-bit dtype: only the bit patterns count)."""
    return np.ascontiguousarray(b).view(np.int8).astype(np.int64)


def out_length(n, L, M):
    return -(-int(n) * int(L) // int(M))


def sums_direct(x, h, L, M):
    """sum_k h[k] u[m M + c - k] for m < ceil(N L / M), u the zero-stuffed record (u[i L] = x[i]); int64.  The contract as
    it is written, tap by tap, stuffed zeros and all."""
    Lh = h.size
    c = (Lh - 1) // 2
    n_out = out_length(x.size, L, M)
    pad = np.zeros(c + max(n_out * M, x.size * L) + c + 1, dtype=np.int64)
    pad[c:c + x.size * L:L] = x              # pad[c + i] = u[i]
    acc = np.zeros(n_out, dtype=np.int64)
    for k in range(Lh):                      # u[m M + c - k] = pad[m M + 2 c - k]
        if h[k]:
            acc += int(h[k]) * pad[2 * c - k:2 * c - k + n_out * M:M][:n_out]
    return acc


def sums_phased(x, h, L, M):
    """sums_direct stream by stream - the same int64 sums without the products with stuffed zeros: for r = m mod L, with
    a = r M + c, phi = a mod L, b = a div L:  y[r + L i] = sum_j h[phi + j L] x[i M + b - j]."""
    Lh = h.size
    c = (Lh - 1) // 2
    n_out = out_length(x.size, L, M)
    acc = np.zeros(n_out, dtype=np.int64)
    for r in range(min(L, n_out)):
        a = r * M + c
        phi, b = a % L, a // L
        g = h[phi::L]
        ni = -(-(n_out - r) // L)            # outputs of this stream
        if g.size == 0 or x.size == 0:
            continue
        full = np.convolve(x, g)             # full[n] = sum_j g[j] x[n - j], n = 0 .. N + J - 2
        at = np.arange(ni, dtype=np.int64) * M + b
        ok = at < full.size
        acc[r::L][ok] = full[at[ok]]
    return acc


def quantise(a, S):
    """(int8 bytes, mask of the clipped ones) of sums a: q(a) = clip((a + (S ? 2^(S-1) : 0)) >> S, -127, 127), and whether
    the value in front of the clip lay outside [-127, 127]."""
    a = np.asarray(a, dtype=np.int64).reshape(-1)
    assert a.size == 0 or np.abs(a).max() < 2 ** 31
    S = int(S)
    if S:
        a = (a + (1 << (S - 1))) >> S        # arithmetic shift: floor
    return np.clip(a, -127, 127).astype(np.int8), (a < -127) | (a > 127)


def resample(b, h, S, L, M, direct=False):
    """(int8 output bytes, clipped): y[m] = q(sum_k h[k] u[m M + c - k]), m < ceil(N L / M); q as quantise(); clipped
    counts the outputs whose value in front of the clip lay outside [-127, 127].  direct: the tap-by-tap form."""
    b = np.ascontiguousarray(b)
    h = np.asarray(h)
    assert b.dtype.itemsize == 1 and h.dtype == np.int16
    check(h, S, L, M)
    form = sums_direct if direct else sums_phased
    y, over = quantise(form(samples(b), h.astype(np.int64), int(L), int(M)), S)
    return y, int(np.count_nonzero(over))


def output_rate(fs, L, M):
    return float(fs) * float(int(L)) / float(int(M))


def default_cutoff(fs, L, M):
    return min(float(fs), output_rate(fs, L, M)) / 2.0


def design_unrounded(fs, L, M, Lh, cutoff=0.0, gain=1.0):
    """The taps in front of the rounding, float64[Lh]: with fu = fs L, fc the cutoff (0: min(fs, fs L / M) / 2), m = k - c
    (2^14 g L) (2 fc / fu) sinc(2 fc m / fu) hann_Lh[k]."""
    fs, cutoff, gain, L, M, Lh = float(fs), float(cutoff), float(gain), int(L), int(M), int(Lh)
    if not (np.isfinite(fs) and fs > 0 and np.isfinite(gain) and gain > 0):
        raise ValueError("fs and gain must be finite and positive")
    if (L, M) not in PAIRS:
        raise ValueError("L / M must be one of the 31 pairs")
    if not (1 <= Lh <= MAX_TAPS and Lh % 2 == 1):
        raise ValueError("n_taps must be odd, 1 .. %d" % MAX_TAPS)
    fu = fs * float(L)
    widest = default_cutoff(fs, L, M)
    if not (np.isfinite(cutoff) and 0 <= cutoff <= widest):
        raise ValueError("the cutoff must lie in 0 .. min(fs, fs L / M) / 2")
    fc = cutoff if cutoff > 0 else widest
    c = (Lh - 1) // 2
    k = np.arange(Lh, dtype=np.float64)
    m = k - c
    t = 2.0 * fc * m / fu
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.sin(np.pi * t) / (np.pi * t)
    sinc[c] = 1.0
    win = np.ones(Lh) if Lh == 1 else 0.5 - 0.5 * np.cos(2.0 * np.pi * k / float(Lh - 1))
    lp = (2.0 * fc / fu) * sinc * win
    return (float(1 << DESIGN_SHIFT) * gain * float(L)) * lp


def design(fs, L, M, Lh=0, cutoff=0.0, gain=1.0):
    """(int16 taps, shift, fs_out): design_unrounded rounded half to even; Lh = 0: default_taps(L); ValueError for a tap
    that resample() does not take."""
    Lh = int(Lh) if Lh else default_taps(L)
    u = np.rint(design_unrounded(fs, L, M, Lh, cutoff, gain))
    if np.abs(u).max() > MAX_TAP or 128 * int(np.abs(u).sum()) >= 2 ** 31:
        raise ValueError("a tap leaves what the resampler takes")
    return u.astype(np.int16), DESIGN_SHIFT, output_rate(fs, L, M)


def rounding_margin(fs, L, M, Lh, cutoff=0.0, gain=1.0):
    """Smallest distance of an unrounded tap from a rounding boundary (k + 1/2)."""
    u = design_unrounded(fs, L, M, Lh, cutoff, gain)
    return float(np.min(np.abs((u - np.floor(u)) - 0.5)))
