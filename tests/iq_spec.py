"""numpy restatement of the I/Q front stage (include/sgx.h: sgx_iq_design, sgx_if_from_iq): the contract the host design
code and the HIP converter kernel (csrc/sgx_iq.hip) are tested against.  Integers only where samples are touched: any
summation order gives the same bytes.  Test infrastructure, not product code."""
import numpy as np

MAX_TAPS = 255
MAX_TAP = 32512          # 127 * 256: every tap splits into two signed bytes, h = 256 hi + lo
DESIGN_SHIFT = 14
Q_FIRST = 1
OFFSET_BINARY = 2
DEFAULT_TAPS = 63        # Settings.iqTaps


def check(h, S, flags=0, n_bytes=0):
    """The preconditions of convert(); the library refuses what fails them with SGX_E_ARG."""
    h = np.asarray(h)
    L = h.size
    if not (1 <= L <= MAX_TAPS and L % 2 == 1):
        raise ValueError("n_taps must be odd, 1 .. %d" % MAX_TAPS)
    if not (0 <= int(S) <= 30):
        raise ValueError("shift must be 0 .. 30")
    a = np.abs(h.astype(np.int64))
    if a.max() > MAX_TAP:
        raise ValueError("|h[k]| must be <= %d" % MAX_TAP)
    if 128 * int(a.sum()) >= 2 ** 31:
        raise ValueError("128 sum|h| must be < 2^31")
    if int(flags) & ~(Q_FIRST | OFFSET_BINARY):
        raise ValueError("unknown flag bits")
    if int(n_bytes) % 2:
        raise ValueError("an I/Q record holds whole pairs: N must be even")


def components(b, flags=0):
    """(I, Q) as int64 from the file's bytes (any 8-bit dtype: only the bit patterns count)."""
    x = np.ascontiguousarray(b).view(np.uint8)
    if int(flags) & OFFSET_BINARY:
        x = x ^ np.uint8(0x80)               # byte - 128, read as int8
    x = x.view(np.int8).astype(np.int64)
    first, second = x[0::2], x[1::2]
    return (second, first) if int(flags) & Q_FIRST else (first, second)


def convert(b, h, S, flags=0):
    """N bytes of interleaved I/Q -> N int8 samples of the real record at twice the rate:
    u[2m] = I[m] + j Q[m], u[odd] = 0, u = 0 outside [0, N);  w[n] = sum_k h[k] u[n + c - k], c = (L - 1) / 2;
    a[n] = Re w, -Im w, -Re w, Im w for n mod 4 = 0, 1, 2, 3;  y[n] = clip((a[n] + (S ? 2^(S-1) : 0)) >> S, -127, 127)."""
    b = np.ascontiguousarray(b)
    h = np.asarray(h)
    assert b.dtype.itemsize == 1 and h.dtype == np.int16
    N = b.size
    check(h, S, flags, N)
    L = h.size
    c = (L - 1) // 2
    I, Q = components(b, flags)
    a = np.zeros(N, dtype=np.int64)
    for comp, first in ((I, 0), (Q, 1)):     # Re w feeds the even outputs, Im w the odd ones
        up = np.zeros(N + 2 * c, dtype=np.int64)
        up[c:c + N:2] = comp                 # up[c + n] = component of u[n]
        acc = np.zeros(N, dtype=np.int64)
        for k in range(L):                   # u[n + c - k] = up[n + 2c - k]
            if h[k]:
                acc += int(h[k]) * up[2 * c - k:2 * c - k + N]
        a[first::2] = acc[first::2]
    assert N == 0 or np.abs(a).max() < 2 ** 31
    a[1::4] = -a[1::4]
    a[2::4] = -a[2::4]
    S = int(S)
    if S:
        a = (a + (1 << (S - 1))) >> S        # arithmetic shift: floor
    return np.clip(a, -127, 127).astype(np.int8)


def design_unrounded(L):
    """2^14 sinc(m / 2) hann_L[k], m = k - c.  sinc(m / 2) in closed form: 1 at m = 0, exactly 0 at every other even m,
    (-1)^((m-1)/2) 2 / (pi m) at odd m."""
    L = int(L)
    assert 1 <= L <= MAX_TAPS and L % 2 == 1
    c = (L - 1) // 2
    m = np.arange(L, dtype=np.int64) - c
    sinc = np.zeros(L)
    odd = (m % 2) == 1
    sinc[odd] = np.where(((m[odd] - 1) // 2) % 2 == 1, -1.0, 1.0) * 2.0 / (np.pi * m[odd].astype(np.float64))
    sinc[c] = 1.0
    win = np.ones(L) if L == 1 else 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L, dtype=np.float64) / (L - 1))
    return float(2 ** DESIGN_SHIFT) * sinc * win


def design(L):
    """(int16 taps, shift): design_unrounded rounded half to even."""
    return np.rint(design_unrounded(L)).astype(np.int16), DESIGN_SHIFT


def rounding_margin(L):
    """Smallest distance of an unrounded tap from a rounding boundary (k + 1/2)."""
    u = design_unrounded(L)
    return float(np.min(np.abs((u - np.floor(u)) - 0.5)))


def real_equivalent(fs_c, if_bb):
    """(samplingFreq, IF) of the converted record."""
    return 2.0 * float(fs_c), float(if_bb) + float(fs_c) / 2.0
