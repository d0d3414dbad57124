"""numpy restatement of the multi-antenna combiner (include/sgx.h: sgx_array_stats, sgx_array_design, sgx_if_combine): the
contract the host design code and the HIP kernels (csrc/sgx_array.hip) are tested against.  Integers only where samples are
touched: any summation order gives the same statistics and the same bytes.  The design runs in Python floats (IEEE
doubles), one operation after the other in the order the header states, so the host code agrees with it to the bit.
Test infrastructure, not product code."""
import math

import numpy as np

from decim_spec import quantise, samples

MAX_ANTENNAS = 8
MAX_TAPS = 15
MAX_WEIGHTS = 64
MAX_TAP = 32512          # 127 * 256: every tap component splits into two signed bytes
DESIGN_SHIFT = 12
OFFSET_BINARY = 1
DEFAULT_LOADING = 1e-3   # Settings.arrayLoading
DEFAULT_TARGET_RMS = 12.0


def check_shape(lanes, A, K, flags=0, n_bytes=0):
    """The preconditions all three functions share; the library refuses what fails them with SGX_E_ARG."""
    if int(lanes) not in (1, 2):
        raise ValueError("lanes must be 1 or 2")
    if not (2 <= int(A) <= MAX_ANTENNAS):
        raise ValueError("A must be 2 .. %d" % MAX_ANTENNAS)
    if not (1 <= int(K) <= MAX_TAPS and int(K) % 2 == 1):
        raise ValueError("K must be odd, 1 .. %d" % MAX_TAPS)
    if int(A) * int(K) > MAX_WEIGHTS:
        raise ValueError("A K must be <= %d" % MAX_WEIGHTS)
    if int(flags) & ~OFFSET_BINARY:
        raise ValueError("unknown flag bits")
    if int(n_bytes) % (int(A) * int(lanes)):
        raise ValueError("the record holds whole frames of A lanes bytes")


def check(h, S, lanes, A, flags=0, n_bytes=0):
    """The preconditions of combine().  h: int16[A, K] for lanes 1, int16[A, K, 2] (re, im) for lanes 2."""
    h = np.asarray(h)
    if h.ndim != (2 if int(lanes) == 1 else 3) or h.shape[0] != int(A) or (int(lanes) == 2 and h.shape[2] != 2):
        raise ValueError("taps are [A, K] or, for I/Q, [A, K, 2]")
    check_shape(lanes, A, h.shape[1], flags, n_bytes)
    if not (0 <= int(S) <= 30):
        raise ValueError("shift must be 0 .. 30")
    a = np.abs(h.astype(np.int64))
    if a.max() > MAX_TAP:
        raise ValueError("a tap component must be <= %d in magnitude" % MAX_TAP)
    if 128 * int(a.sum()) >= 2 ** 31:
        raise ValueError("128 sum|h| must be < 2^31 (over all antennas; lanes 2: the sum of |re| + |im|)")


def streams(b, lanes, A, flags=0):
    """The record's bytes as int64[F, A, lanes]."""
    x = samples(b, flags)
    return x.reshape(-1, int(A), int(lanes))


def _dot(u, v):
    """u^T v of two integer matrices of small entries, exact: float64 sums of integers below 2^53 are exact in any order."""
    assert u.shape[0] * 2 * 128 * 128 < 2 ** 52
    return np.rint(u.astype(np.float64).T @ v.astype(np.float64)).astype(np.int64)


def stats(b, lanes, A, K, flags=0):
    """int64 rho[A, A, K, lanes]: rho[a, b, d] = sum_{f = 0}^{F-1-d} x_a[f + d] conj(x_b[f]), the real part, then (lanes 2)
    the imaginary part."""
    b = np.ascontiguousarray(b)
    check_shape(lanes, A, K, flags, b.size)
    x = streams(b, lanes, A, flags)
    F = x.shape[0]
    rho = np.zeros((A, A, K, lanes), dtype=np.int64)
    for d in range(min(K, F)):
        lead, lag = x[d:], x[:F - d]
        if lanes == 1:
            rho[:, :, d, 0] = _dot(lead[:, :, 0], lag[:, :, 0])
        else:
            (ai, aq), (bi, bq) = (lead[:, :, 0], lead[:, :, 1]), (lag[:, :, 0], lag[:, :, 1])
            rho[:, :, d, 0] = _dot(ai, bi) + _dot(aq, bq)
            rho[:, :, d, 1] = _dot(aq, bi) - _dot(ai, bq)
    return rho


def covariance(rho, frames, lanes):
    """(P, Q) of step 1, lists of lists of floats: R = P + j Q, R[(a,k)][(b,l)] = rho_ab[l - k] / frames."""
    rho = np.asarray(rho, dtype=np.int64)
    A, K = rho.shape[0], rho.shape[2]
    n, fr = A * K, float(int(frames))
    P = [[0.0] * n for _ in range(n)]
    Q = [[0.0] * n for _ in range(n)]
    for a in range(A):
        for k in range(K):
            for b in range(A):
                for l in range(K):
                    d = l - k
                    e = rho[a, b, d] if d >= 0 else rho[b, a, -d]
                    P[a * K + k][b * K + l] = float(int(e[0])) / fr
                    if lanes == 2:
                        q = float(int(e[1])) / fr
                        Q[a * K + k][b * K + l] = q if d >= 0 else -q
    return P, Q


def loaded_system(rho, frames, lanes, loading):
    """(M, m): the real symmetric matrix of step 3 (lists of lists) and its order."""
    P, Q = covariance(rho, frames, lanes)
    n = len(P)
    tr = 0.0
    for i in range(n):
        tr += P[i][i]
    ld = (float(loading) * tr) / float(n)
    m = lanes * n
    M = [[0.0] * m for _ in range(m)]
    for i in range(n):
        for j in range(n):
            p = P[i][j] + (ld if i == j else 0.0)
            M[i][j] = p
            if lanes == 2:
                M[i][n + j] = -Q[i][j]
                M[n + i][j] = Q[i][j]
                M[n + i][n + j] = p
    return M, m


def design(rho, frames, lanes, ref=0, loading=DEFAULT_LOADING, target_rms=DEFAULT_TARGET_RMS):
    """(taps int16[A, K] or [A, K, 2], shift, gain, suppression_db, weights float64[A, K] or complex128[A, K]): the
    power-inversion design, steps 1 .. 9 of the header in its order; ValueError for what the library refuses."""
    rho = np.asarray(rho)
    lanes = int(lanes)
    if rho.ndim != 4 or rho.shape[0] != rho.shape[1] or rho.shape[3] != lanes:
        raise ValueError("rho is [A, A, K, lanes]")
    A, K = rho.shape[0], rho.shape[2]
    check_shape(lanes, A, K)
    if not (0 <= int(ref) < A):
        raise ValueError("ref must be one of the antennas")
    loading, target_rms = float(loading), float(target_rms)
    if not (math.isfinite(loading) and loading >= 0):
        raise ValueError("loading must be finite and >= 0")
    if not (0 < target_rms <= 127.0):
        raise ValueError("target_rms must lie in (0, 127]")
    if int(frames) < 1:
        raise ValueError("frames must be >= 1")
    n, c = A * K, (K - 1) // 2
    at = int(ref) * K + c
    P, Q = covariance(rho, frames, lanes)
    M, m = loaded_system(rho, frames, lanes, loading)
    for j in range(m):
        Mj = M[j]
        for i in range(j, m):
            Mi = M[i]
            s = Mi[j]
            for k in range(j):
                s -= Mi[k] * Mj[k]
            if i == j:
                if not s > 0:
                    raise ValueError("the covariance matrix is not positive definite")
                Mj[j] = math.sqrt(s)
            else:
                Mi[j] = s / Mj[j]
    y, g = [0.0] * m, [0.0] * m
    for i in range(m):
        s = 1.0 if i == at else 0.0
        for k in range(i):
            s -= M[i][k] * y[k]
        y[i] = s / M[i][i]
    for i in range(m - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, m):
            s -= M[k][i] * g[k]
        g[i] = s / M[i][i]
    g0 = g[at]
    if not (math.isfinite(g0) and g0 > 0):
        raise ValueError("the covariance matrix is not positive definite")
    g = [v / g0 for v in g]
    gr, gi = g[:n], g[n:]
    p_out = 0.0
    for i in range(n):
        t_re, t_im = 0.0, 0.0
        for j in range(n):
            t_re += P[i][j] * gr[j]
            if lanes == 2:
                t_re -= Q[i][j] * gi[j]
                t_im += P[i][j] * gi[j]
                t_im += Q[i][j] * gr[j]
        p_out += gr[i] * t_re
        if lanes == 2:
            p_out += gi[i] * t_im
    if not (math.isfinite(p_out) and p_out > 0):
        raise ValueError("the covariance matrix is not positive definite")
    gain = target_rms / math.sqrt(p_out / float(lanes))
    scale = float(1 << DESIGN_SHIFT) * gain
    h = np.zeros((A, K, lanes))
    for i in range(n):
        h[i // K, i % K, 0] = gr[i]
        if lanes == 2:
            h[i // K, i % K, 1] = -gi[i]
    u = np.rint(scale * h)
    if np.abs(u).max() > MAX_TAP:
        raise ValueError("a tap leaves what the combiner takes")
    if 128 * int(np.abs(u).sum()) >= 2 ** 31:
        raise ValueError("128 sum|h| leaves the int32 accumulator")
    supp = 10.0 * math.log10(P[at][at] / p_out)
    if lanes == 2:
        return u.astype(np.int16), DESIGN_SHIFT, gain, supp, h[:, :, 0] + 1j * h[:, :, 1]
    return u[:, :, 0].astype(np.int16), DESIGN_SHIFT, gain, supp, h[:, :, 0].copy()


def _fir(x, h, F):
    """sum_k h[k] x[f + c - k], f < F, x = 0 outside; int64."""
    c = (h.size - 1) // 2
    if F == 0:
        return np.zeros(0, dtype=np.int64)
    return np.convolve(x, h)[c:c + F]


def sums(b, h, lanes, A, flags=0):
    """The sums in front of the rounding, int64: [F] for lanes 1, [F, 2] (Re w, Im w) for lanes 2."""
    x = streams(b, lanes, A, flags)
    h = np.asarray(h).astype(np.int64)
    F = x.shape[0]
    if lanes == 1:
        acc = np.zeros(F, dtype=np.int64)
        for a in range(A):
            acc += _fir(x[:, a, 0], h[a], F)
        return acc
    re, im = np.zeros(F, dtype=np.int64), np.zeros(F, dtype=np.int64)
    for a in range(A):
        I, Q, hr, hi = x[:, a, 0], x[:, a, 1], h[a, :, 0], h[a, :, 1]
        re += _fir(I, hr, F) - _fir(Q, hi, F)
        im += _fir(Q, hr, F) + _fir(I, hi, F)
    return np.stack([re, im], axis=1)


def combine(b, h, S, lanes, A, flags=0):
    """(int8 output bytes, clipped).  lanes 1: y[f] = q(sum_a sum_k h_a[k] x_a[f + c - k]); lanes 2: w[f] = sum_a sum_k
    h_a[k] z_a[f + c - k] with complex h, bytes q(Re w[f]), q(Im w[f]).  q as decim_spec.quantise; clipped counts the
    output bytes whose value in front of the clip lay outside [-127, 127]."""
    b = np.ascontiguousarray(b)
    h = np.asarray(h)
    assert b.dtype.itemsize == 1 and h.dtype == np.int16
    check(h, S, lanes, A, flags, b.size)
    y, over = quantise(sums(b, h, lanes, A, flags), S)
    return y, int(np.count_nonzero(over))


def input_rms(rho, frames):
    """rms per component of every antenna, from rho[a][a][0]."""
    rho = np.asarray(rho)
    lanes = rho.shape[3]
    return np.sqrt(np.array([float(rho[a, a, 0, 0]) for a in range(rho.shape[0])]) / (float(frames) * lanes))
