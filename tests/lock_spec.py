"""numpy restatement of the C/N0 estimate and lock detector (include/sgx.h, sgx_track_quality): the contract the HIP
kernel of csrc/sgx_quality.hip is tested against.  Test infrastructure only; the package never imports it.

For channel c the prompt series I_P[c][k], Q_P[c][k], k < ms_done[c], are cut into windows of W ms (window j covers
k = jW .. jW+W-1, j < n_c = ms_done[c] // W; a trailing partial window is dropped).  Over each window, in fp64:

    R = sum(I^2 - Q^2)   X = sum(2 I Q)   P = sum(I^2 + Q^2)
    phi = atan2(X, R) / 2                        the window's carrier phase error from the squared prompt
    A = sum |I cos phi + Q sin phi|              the prompt rotated onto the in-phase axis
    Psig = (A / W)^2   Ptot = P / W
    CNo = 10 log10(Psig / ((Ptot - Psig) T))     dB-Hz; NaN for P = 0, -inf for Psig = 0 < P, +inf for Ptot - Psig <= 0 < Psig
    carrLock = R / sqrt(R^2 + X^2) = cos 2 phi   NaN for R = X = 0
    pass = CNo >= cnoThreshold and carrLock >= carrLockThreshold   (a NaN fails)

The counter f starts at 0, becomes f + 1 on a fail and max(f - 1, 0) on a pass, window by window; lost is the first j
with f >= maxLockFail, or -1.  Windows j >= n_c report NaN, NaN and pass 0, and the counter does not see them.
"""
import numpy as np


def window_stats(i, q, W):
    """(CNo, carrLock) of the whole windows of one channel's series i, q (T = 1 for the CNo here: see quality())."""
    n = len(i) // W
    I = np.asarray(i[:n * W], dtype=np.float64).reshape(n, W)
    Q = np.asarray(q[:n * W], dtype=np.float64).reshape(n, W)
    R = np.sum(I * I - Q * Q, axis=1)
    X = np.sum(2.0 * I * Q, axis=1)
    P = np.sum(I * I + Q * Q, axis=1)
    phi = 0.5 * np.arctan2(X, R)
    A = np.sum(np.abs(I * np.cos(phi)[:, None] + Q * np.sin(phi)[:, None]), axis=1)
    return R, X, P, A


def cno_carr_lock(R, X, P, A, W, T):
    psig = (A / W) ** 2
    ptot = P / W
    with np.errstate(divide="ignore", invalid="ignore"):
        cno = 10.0 * np.log10(psig / ((ptot - psig) * T))
        cl = R / np.sqrt(R * R + X * X)
    cno = np.where(P == 0, np.nan, np.where(psig == 0, -np.inf, np.where(ptot - psig <= 0, np.inf, cno)))
    return cno, cl


def lock_scan(passes, max_fail):
    """First window at which the fail counter reaches max_fail, or -1."""
    f = 0
    for j, ok in enumerate(passes):
        f = max(f - 1, 0) if ok else f + 1
        if f >= max_fail:
            return j
    return -1


def quality(i_p, q_p, T, cno_min, carr_lock_min, W, max_fail, ms_done=None):
    """(cno, carr_lock, pass, lost) with the shapes of sgx_track_quality: [n_ch, ms // W] x 3 and [n_ch]."""
    i_p = np.asarray(i_p, dtype=np.float64)
    q_p = np.asarray(q_p, dtype=np.float64)
    n_ch, ms = i_p.shape
    nw = ms // W
    cno = np.full((n_ch, nw), np.nan)
    cl = np.full((n_ch, nw), np.nan)
    ok = np.zeros((n_ch, nw), dtype=bool)
    lost = np.full(n_ch, -1, dtype=np.int64)
    for c in range(n_ch):
        done = ms if ms_done is None else int(ms_done[c])
        n_c = done // W
        R, X, P, A = window_stats(i_p[c, :n_c * W], q_p[c, :n_c * W], W)
        cno[c, :n_c], cl[c, :n_c] = cno_carr_lock(R, X, P, A, W, T)
        with np.errstate(invalid="ignore"):
            ok[c, :n_c] = (cno[c, :n_c] >= cno_min) & (cl[c, :n_c] >= carr_lock_min)
        lost[c] = lock_scan(ok[c, :n_c], max_fail)
    return cno, cl, ok, lost


def synthetic_prompts(rng, n_ms, cno_dbhz, phase, sigma=100.0, T=1e-3, bit_ms=20):
    """Complex prompts A d_k e^{j phase} + noise with random data bits d_k (one per bit_ms) and a noise of sigma per
    component, A chosen so that 10 log10(A^2 / (2 sigma^2 T)) = cno_dbhz.  Returns (I, Q)."""
    A = np.sqrt(2.0 * sigma ** 2 * T * 10.0 ** (cno_dbhz / 10.0))
    bits = rng.choice([-1.0, 1.0], size=(n_ms + bit_ms - 1) // bit_ms)
    d = np.repeat(bits, bit_ms)[:n_ms]
    z = A * d * np.exp(1j * phase) + sigma * (rng.standard_normal(n_ms) + 1j * rng.standard_normal(n_ms))
    return z.real, z.imag
