"""numpy restatement of the record monitor (include/sgx.h: sgx_probe_waterfall, sgx_waterfall_plan): the contract the HIP
kernels of csrc/sgx_waterfall.hip and the host code around them (frontend.py: monitorRecord) are tested against.  Plain
numpy, no product import.  Test infrastructure, not product code.

A window [offset, offset + n) of an int8 record is cut into slices of S samples; each slice gives a Welch spectrum of its
own (segments of N samples, noverlap shared, constant detrend, periodic Hamming window, density scaling, one-sided) and the
exact integer statistics of all its samples."""
import numpy as np

MIN_SEGMENT, MAX_SEGMENT = 256, 16384
MAX_SLICE = 2 ** 32          # samples of a slice: 2^32 * 127^4 < 2^63, so the sum of x^4 of a slice fits int64


def check(n, N, noverlap, S):
    """The preconditions; the library refuses what fails them (SGX_E_ARG; n < N: SGX_E_RANGE, as sgx_probe_stats)."""
    N, noverlap, S = int(N), int(noverlap), int(S)
    if not (MIN_SEGMENT <= N <= MAX_SEGMENT and N & (N - 1) == 0):
        raise ValueError("the segment length is a power of two in %d .. %d" % (MIN_SEGMENT, MAX_SEGMENT))
    if not 0 <= noverlap < N:
        raise ValueError("noverlap lies in [0, N)")
    if not N <= S <= MAX_SLICE:
        raise ValueError("a slice holds at least one segment and at most 2^32 samples")
    if int(n) < N:
        raise ValueError("the window holds less than one segment")


def plan(n, N, noverlap, S):
    """[(start, length, segments)] of the slices that are kept, start relative to the window: slice j covers [j S,
    min((j + 1) S, n)); a trailing piece shorter than N is dropped."""
    check(n, N, noverlap, S)
    step = N - noverlap
    out = []
    for start in range(0, n, S):
        length = min(S, n - start)
        if length < N:
            break
        out.append((start, length, (length - noverlap) // step))
    return out


def window(N):
    """Periodic Hamming: scipy.signal.get_window('hamming', N, fftbins=True)."""
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(N) / N)


def segment_spectrum(seg, w):
    """|rfft(w d)|^2 of one segment, d[i] = (N x[i] - sum x) / N from the exact integer numerator."""
    N = seg.size
    x = seg.astype(np.int64)
    d = (N * x - int(x.sum())).astype(np.float64) / float(N)
    X = np.fft.rfft(w * d)
    return X.real * X.real + X.imag * X.imag


def slice_stats(xs):
    """(moments int64[4] = count, sum x, sum x^2, sum x^4; hist int64[256], -128 in bin 0) of a slice's samples."""
    v = xs.astype(np.int64)
    v2 = v * v
    return (np.array([v.size, v.sum(), v2.sum(), (v2 * v2).sum()], dtype=np.int64),
            np.bincount(v + 128, minlength=256).astype(np.int64))


def waterfall(x, offset, n, fs_mhz, N, noverlap, S):
    """dict(f[N/2+1] MHz, pxx[n_slices][N/2+1], hold[N/2+1], moments int64[n_slices][4], hist int64[n_slices][256],
    n_segments int64[n_slices]) of samples [offset, offset + n) of the int8 record x."""
    x = np.asarray(x)
    assert x.dtype == np.int8 and 0 <= offset and offset + n <= x.size
    slices = plan(n, N, noverlap, S)
    step, bins = N - noverlap, N // 2 + 1
    w = window(N)
    scale = 1.0 / (fs_mhz * float((w * w).sum()))
    two = np.ones(bins)
    two[1:bins - 1] = 2.0
    pxx = np.zeros((len(slices), bins))
    moments = np.zeros((len(slices), 4), dtype=np.int64)
    hist = np.zeros((len(slices), 256), dtype=np.int64)
    for j, (start, length, K) in enumerate(slices):
        xs = x[offset + start:offset + start + length]
        acc = np.zeros(bins)
        for i in range(K):                                   # in segment order
            acc += (segment_spectrum(xs[i * step:i * step + N], w) * scale) * two
        pxx[j] = acc / float(K)
        moments[j], hist[j] = slice_stats(xs)
    f = np.arange(bins) * (1.0 / (N * (1.0 / fs_mhz)))       # np.fft.rfftfreq(N, 1 / fs), as sgx_probe_stats
    return dict(f=f, pxx=pxx, hold=pxx.max(axis=0), moments=moments, hist=hist,
                n_segments=np.array([s[2] for s in slices], dtype=np.int64))


def derived(moments, hist):
    """(mean, rms, kurtosis, clip_share) per slice, float64 from the integers: rms = sqrt(sum x^2 / n); the excess
    kurtosis m4 / m2^2 - 3 about the mean (0 where the slice is constant); the share of samples on -128, -127 or +127."""
    m = np.asarray(moments, dtype=np.int64)
    h = np.asarray(hist, dtype=np.int64)
    n = m[:, 0].astype(np.float64)
    mean = m[:, 1] / n
    e2, e4 = m[:, 2] / n, m[:, 3] / n
    # the third raw moment comes from the histogram (exact integers)
    v = np.arange(-128, 128, dtype=np.int64)
    e3 = (h * v ** 3).sum(axis=1) / n
    m2 = e2 - mean * mean
    m4 = e4 - 4.0 * mean * e3 + 6.0 * mean * mean * e2 - 3.0 * mean ** 4
    with np.errstate(divide="ignore", invalid="ignore"):
        kurt = np.where(m2 > 0, m4 / (m2 * m2) - 3.0, 0.0)
    clip = (h[:, 0] + h[:, 1] + h[:, 255]) / n
    return mean, np.sqrt(e2), kurt, clip


# ---- events and pulsed slices (frontend.py: monitorRecord) -------------------------------------------------------------
PULSED_MADS = 6.0


def merge_events(per_slice, slice_ms, min_slices):
    """per_slice[j]: the lines (f_hz, width_hz, peak_db) of slice j in ascending frequency.  A line continues an event
    whose last slice is j - 1 when their bands [f - w/2, f + w/2] overlap (the first such event in order of creation);
    else it opens one.  An event's f_hz and peak_db are those of its strongest slice, its width the widest; first_ms =
    first slice * slice_ms, last_ms = (last slice + 1) * slice_ms.  Events of fewer than min_slices slices are dropped;
    the rest are returned in order of (first_ms, f_hz) as (f_hz, width_hz, first_ms, last_ms, peak_db)."""
    events = []          # [f, w, first, last, peak, band_lo, band_hi]
    for j, lines in enumerate(per_slice):
        for f, w, peak in lines:
            lo, hi = f - w / 2.0, f + w / 2.0
            for e in events:
                if e[3] == j - 1 and lo <= e[6] and e[5] <= hi:
                    if peak > e[4]:
                        e[0], e[4] = f, peak
                    e[1], e[3], e[5], e[6] = max(e[1], w), j, lo, hi
                    break
            else:
                events.append([f, w, j, j, peak, lo, hi])
    out = [(e[0], e[1], e[2] * slice_ms, (e[3] + 1) * slice_ms, e[4]) for e in events if e[3] - e[2] + 1 >= min_slices]
    return sorted(out, key=lambda e: (e[2], e[0]))


def pulsed(kurtosis, clip_share, mads=PULSED_MADS):
    """Indices of the slices whose excess kurtosis or clip share exceeds median + mads * 1.4826 * MAD of that figure over
    the record's own slices (strictly: with a spread of 0 nothing equal to the median is flagged)."""
    flagged = np.zeros(len(kurtosis), dtype=bool)
    for v in (np.asarray(kurtosis, dtype=np.float64), np.asarray(clip_share, dtype=np.float64)):
        if v.size:
            med = np.median(v)
            mad = np.median(np.abs(v - med))
            flagged |= v > med + mads * 1.4826 * mad
    return [int(j) for j in np.nonzero(flagged)[0]]
