"""numpy statement of the swept-interference excision stage (include/sgx.h: sgx_if_excise, sgx_excise_host): the contract
the host items and the HIP kernel (csrc/sgx_excise_core.h, csrc/sgx_excise.hip) are tested against.  Test infrastructure,
not product code.

A real int8 record x of n >= 1 samples, segment length N (a power of two in 64 .. 1024), hop H = N / 2:
  segment j = 0 .. J - 1, J = ceil(n / H) + 1, covers samples [(j - 1) H, (j + 1) H), zero outside [0, n);
  w[i] = sin(pi i / N) (periodic root-Hann: w[i]^2 + w[i + H]^2 = 1);  X = rfft(w * segment), P_k = |X_k|^2;
  candidates k = 1 .. N/2 - 1; kept = all candidates, then `passes` times: m = mean(P[kept]), kept = {k: P_k <= threshold m};
  X_k = 0 on the candidates outside kept, xt = irfft(X), o[(j - 1) H + i] += w[i] xt[i] in segment order;
  y = clip(floor(o + 1/2), -127, 127), the rounding of tests/notch_spec.py's apply ((acc + 2^(S-1)) >> S is floor(v + 1/2));
  clipped counts the samples whose rounded value lay outside [-127, 127] in front of the clip.

The margin.  The library's transform is another algorithm than numpy's, so its bytes equal the contract's only where no
decision sits on a rounding error.  Every case of tests/excise_cases.py keeps MARGIN = 1e-9 clear of every decision:
relative to threshold m in every comparison, absolute from a half-integer for every o.  The standard bound for the
error of a power-of-two FFT in fp64 is c log2(N) 2^-53 max|value| with c a small constant; c = 8 covers the radix-2 .. 16
butterflies, the tabulated twiddles and the real-input split on top.  At N = 1024 on int8 input:
  forward:  max|X| <= 127 N = 130 048          -> 8 x 10 x 2^-53 x 130 048 = 1.2e-9 on a spectrum value, relative to the
            largest one 8 x 10 x 2^-53 = 8.9e-15; P_k = |X_k|^2 doubles that, and a bin 1e4 below the largest in power
            (the tables hold no chirp stronger over the kept bins) carries it 100-fold: 1.8e-12 relative, m likewise;
  inverse:  the same bound on X / N (the 1 / N scaling is exact) is 1.2e-12 in the samples, its own 8 x 10 x 2^-53 x 127 =
            1.1e-12 adds to it, the window and the two-term overlap-add add 3 x 2^-53 x 254: 2.3e-12 + 1e-13 in o.
Both are more than 100 times below 1e-9 (the larger, 2.4e-12, 416 times).  tests/test_excise_host.py measures the
difference of the host items' spectra from numpy.fft.rfft and holds it to the same factor."""
import numpy as np

MIN_SEGMENT = 64
MAX_SEGMENT = 1024
MAX_PASSES = 8
MARGIN = 1e-9
FFT_BOUND_C = 8.0


def fft_error_bound(N=MAX_SEGMENT):
    """(relative error of a comparison, absolute error of o) by the bound in this file's head."""
    u, lg = 2.0 ** -53, np.log2(float(N))
    fwd_rel = FFT_BOUND_C * lg * u                       # of a spectrum value, relative to the largest
    cmp_rel = 2.0 * fwd_rel * 100.0                      # |X|^2, on a bin 1e4 below the largest in power
    inv_abs = FFT_BOUND_C * lg * u * 127.0               # each of: the forward error carried through, the inverse's own
    ola_abs = 3.0 * u * 254.0
    return cmp_rel, 2.0 * inv_abs + ola_abs


def check(n, N, threshold, passes):
    """The preconditions; the library refuses what fails them with SGX_E_ARG."""
    N = int(N)
    if not (MIN_SEGMENT <= N <= MAX_SEGMENT and N & (N - 1) == 0):
        raise ValueError("N must be a power of two in %d .. %d" % (MIN_SEGMENT, MAX_SEGMENT))
    if not (np.isfinite(threshold) and threshold >= 1.0):
        raise ValueError("threshold must be finite and >= 1")
    if not (1 <= int(passes) <= MAX_PASSES):
        raise ValueError("passes must be 1 .. %d" % MAX_PASSES)
    if int(n) < 1:
        raise ValueError("the record must hold a sample")


def segments(n, N):
    """J = ceil(n / H) + 1."""
    H = int(N) // 2
    return -(-int(n) // H) + 1


def window(N):
    return np.sin(np.pi * np.arange(int(N), dtype=np.float64) / float(N))


def excise(x, N=256, threshold=8.0, passes=3, margins=False):
    """(y int8, info) of the contract.  info: segments, bins_cut, segments_cut, clipped, cut_per_segment (uint16[J]).  With
    margins=True also info['margin_compare'] (the smallest |P_k - threshold m| / (threshold m) over every comparison of every
    pass, inf where there is none; a segment whose powers are all exactly 0 compares 0 <= 0 in any arithmetic and is left
    out) and info['margin_round'] (the smallest distance of an o from a half-integer - which covers the ties at the clip
    rails, +-127.5, too)."""
    x = np.asarray(x)
    assert x.dtype == np.int8 and x.ndim == 1
    n, N, passes, threshold = x.size, int(N), int(passes), float(threshold)
    check(n, N, threshold, passes)
    H = N // 2
    J = segments(n, N)
    xp = np.zeros((J + 1) * H)
    xp[H:H + n] = x                                       # xp[H + s] = sample s: segment j is xp[j H : j H + N]
    w = window(N)
    seg = np.lib.stride_tricks.as_strided(xp, shape=(J, N), strides=(H * xp.strides[0], xp.strides[0]))
    X = np.fft.rfft(seg * w, axis=1)
    P = (X.real * X.real + X.imag * X.imag)[:, 1:H]       # the candidates
    kept = np.ones(P.shape, dtype=bool)
    margin = np.inf
    for _ in range(passes):
        m = np.array([row[k].mean() for row, k in zip(P, kept)])      # (kept is never empty)
        tm = threshold * m
        kept = P <= tm[:, None]
        if margins:
            live = tm > 0.0
            if live.any():
                margin = min(margin, float(np.min(np.abs(P[live] - tm[live, None]) / tm[live, None])))
    cut = ~kept
    X[:, 1:H][cut] = 0.0
    xt = np.fft.irfft(X, n=N, axis=1) * w
    o = np.zeros((J + 1) * H)
    for j in range(J):                                    # segment order: each sample takes its two terms in this order
        o[j * H:j * H + N] += xt[j]
    o = o[H:H + n]
    q = np.floor(o + 0.5)
    per = cut.sum(axis=1)
    info = dict(segments=J, bins_cut=int(per.sum()), segments_cut=int(np.count_nonzero(per)),
                clipped=int(np.count_nonzero((q < -127) | (q > 127))), cut_per_segment=per.astype(np.uint16))
    if margins:
        info["margin_compare"] = margin
        info["margin_round"] = float(np.min(np.abs((o - np.floor(o)) - 0.5)))
    return np.clip(q, -127, 127).astype(np.int8), info
