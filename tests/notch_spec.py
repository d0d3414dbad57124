"""numpy restatement of the interference-excision stage (include/sgx.h: sgx_notch_design, sgx_if_filter): the contract the
host design code and the HIP filter kernel (csrc/sgx_notch.cpp, csrc/sgx_filter.hip) are tested against.  Integers only
where samples are touched: any summation order gives the same bytes.  Test infrastructure, not product code."""
import numpy as np

MAX_TAPS = 4095
MAX_TAP = 32512          # 127 * 256: every tap splits into two signed bytes, h = 256 hi + lo
MAX_LINES = 8
HALF_WINDOW = 128        # bins either side of a bin that its baseline's median is taken over
MERGE_GAP = 2            # flagged bins this many unflagged bins apart (or closer) belong to one line
DESIGN_SHIFT = 14


def check(h, S):
    """The preconditions of apply(); the library refuses what fails them with SGX_E_ARG."""
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


def split(h):
    """(hi, lo) signed bytes with h = 256 hi + lo."""
    h = np.asarray(h, dtype=np.int64)
    hi = (h + 128) >> 8
    return hi.astype(np.int8), (h - 256 * hi).astype(np.int8)


def apply(x, h, S):
    """y[n] = clip((sum_k h[k] x[n + c - k] + (S ? 2^(S-1) : 0)) >> S, -127, 127), c = (L-1)/2, x = 0 outside the record."""
    x = np.asarray(x)
    h = np.asarray(h)
    assert x.dtype == np.int8 and h.dtype == np.int16
    check(h, S)
    L, N = h.size, x.size
    c = (L - 1) // 2
    xp = np.zeros(N + 2 * c, dtype=np.int64)
    xp[c:c + N] = x
    acc = np.zeros(N, dtype=np.int64)
    for k in range(L):                      # x[n + c - k] = xp[n + 2c - k]
        if h[k]:
            acc += int(h[k]) * xp[2 * c - k:2 * c - k + N]
    assert N == 0 or np.abs(acc).max() < 2 ** 31
    S = int(S)
    if S:
        acc = (acc + (1 << (S - 1))) >> S   # arithmetic shift: floor
    return np.clip(acc, -127, 127).astype(np.int8)


def baseline(pxx):
    """b[i] = median(pxx[max(0, i-128) : min(n, i+129)]); an even count takes the mean of the two middle values."""
    p = np.asarray(pxx, dtype=np.float64)
    n = p.size
    b = np.empty(n)
    for i in range(n):
        w = np.sort(p[max(0, i - HALF_WINDOW):min(n, i + HALF_WINDOW + 1)])
        m = w.size
        b[i] = w[m // 2] if m & 1 else 0.5 * (w[m // 2 - 1] + w[m // 2])
    return b


def detect(f_mhz, pxx, threshold_db, width_hz=80e3):
    """Narrowband lines of a one-sided PSD: [(centre Hz, width Hz)] in ascending frequency, at most 8 (the strongest by
    peak / baseline, the lower bin first among equals).  Bin i is flagged when pxx[i] > 10^(threshold_db / 10) b[i];
    flagged bins with at most 2 unflagged bins between them form one line; its centre is the frequency of its largest bin
    (the first of equals) and its width max(width_hz, (f[last] - f[first]) 1e6 + 2 bin widths)."""
    f = np.asarray(f_mhz, dtype=np.float64)
    p = np.asarray(pxx, dtype=np.float64)
    n = p.size
    assert f.size == n and n >= 2
    thr = 10.0 ** (float(threshold_db) / 10.0)
    b = baseline(p)
    idx = np.flatnonzero(p > thr * b)
    df = (float(f[1]) - float(f[0])) * 1e6
    runs = []
    for i in idx:
        if runs and i - runs[-1][1] <= MERGE_GAP + 1:
            runs[-1][1] = int(i)
        else:
            runs.append([int(i), int(i)])
    found = []
    for first, last in runs:
        peak = first + int(np.argmax(p[first:last + 1]))
        strength = float("inf") if b[peak] == 0.0 else float(p[peak]) / float(b[peak])
        width = max(float(width_hz), (float(f[last]) - float(f[first])) * 1e6 + 2.0 * df)
        found.append((peak, strength, float(f[peak]) * 1e6, width))
    if len(found) > MAX_LINES:
        found = sorted(found, key=lambda t: -t[1])[:MAX_LINES]     # stable: the lower bin first among equals
        found.sort(key=lambda t: t[0])
    return [(t[2], t[3]) for t in found]


def design_unrounded(lines, fs, L, S=DESIGN_SHIFT):
    """2^S hann(L) h_ideal before rounding, with m = k - c:
    h_ideal[k] = delta[m] - sum_i 2 (w_i / fs) sinc(w_i m / fs) cos(2 pi f_i m / fs),  sinc(t) = sin(pi t) / (pi t)."""
    L = int(L)
    assert 1 <= L <= MAX_TAPS and L % 2 == 1
    c = (L - 1) // 2
    m = np.arange(L, dtype=np.float64) - c
    h = np.zeros(L)
    h[c] = 1.0
    for f_i, w_i in lines:
        t = float(w_i) * m / float(fs)
        with np.errstate(invalid="ignore", divide="ignore"):
            sinc = np.where(m == 0, 1.0, np.sin(np.pi * t) / (np.pi * t))
        h = h - 2.0 * (float(w_i) / float(fs)) * sinc * np.cos(2.0 * np.pi * float(f_i) * m / float(fs))
    win = np.ones(L) if L == 1 else 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L, dtype=np.float64) / (L - 1))
    return h * win * float(2 ** int(S))


def design(lines, fs, L, S=DESIGN_SHIFT):
    """int16 taps: design_unrounded rounded half to even."""
    u = design_unrounded(lines, fs, L, S)
    assert np.abs(u).max() <= MAX_TAP
    return np.rint(u).astype(np.int16)


def rounding_margin(lines, fs, L, S=DESIGN_SHIFT):
    """Smallest distance of an unrounded tap from a rounding boundary (k + 1/2)."""
    u = design_unrounded(lines, fs, L, S)
    return float(np.min(np.abs((u - np.floor(u)) - 0.5)))
