"""numpy restatement of the coherent multi-millisecond acquisition (include/sgx.h, sgx_acquire_coherent): the contract the
HIP path is checked against.  It extends the reference's search (acquisition.py:62-193; oracle.acquire is its numpy form)
with T_c-ms windows folded on a finer Doppler grid.  Test infrastructure only; written for small searches."""
import numpy as np

from oracle import softgnss_oracle as orc

MAX_MS = 20
MAX_WINDOWS = 64
MAX_SPAN_MS = 400
MAX_BINS = 1024
MAX_PHI = 64
MAX_ROWS = 2048            # direct path: windows x bins
CHUNK_ROWS = 348           # correlation rows per batch
FFT4_N = 38192             # the four-step transform's length (the shift path needs it)


class ArgError(ValueError):
    pass


def default_step(coherent_ms):
    return 500.0 / coherent_ms


def grid(s, coherent_ms=1, n_windows=2, noncoh=False, bin_step_hz=None):
    """Doppler grid, phi decomposition, path and batches of a search (sgx_acquire_coherent_plan).  ArgError where the
    library returns SGX_E_ARG."""
    T, M = int(coherent_ms), int(n_windows)
    step = default_step(T) if bin_step_hz is None and T > 0 else bin_step_hz
    if not (1 <= T <= MAX_MS and 1 <= M <= MAX_WINDOWS and T * M <= MAX_SPAN_MS):
        raise ArgError("coherent_ms x n_windows out of range")
    if step is None or not np.isfinite(step) or not step > 0:
        raise ArgError("bin_step_hz must be > 0")
    nb = np.round(s.acqSearchBand * 1000.0 / step) + 1
    if not 1 <= nb <= MAX_BINS:
        raise ArgError("too many Doppler bins")
    n_bins = int(nb)
    N = s.samplesPerCode
    f0 = s.IF - s.acqSearchBand / 2 * 1000
    freqs = np.array([f0 + step * k for k in range(n_bins)])
    phis, phi_index, shift = [], [], []
    for f in freqs:
        ratio = f * float(N) / s.samplingFreq
        sh = np.floor(ratio + 1e-9)
        phi = ratio - sh
        if phi < 1e-9:
            phi = 0.0
        j = [q for q in range(len(phis)) if abs(phis[q] - phi) < 1e-9]
        if not j:
            phis.append(phi)
            j = [len(phis) - 1]
        phi_index.append(j[0])
        shift.append(int(sh) % N)
    n_phi = len(phis)
    path = "shift" if N == FFT4_N and n_phi <= MAX_PHI else "direct"
    if path == "direct" and M * n_bins > MAX_ROWS:
        raise ArgError("direct path: too many windows x bins")
    rows = M * n_bins
    per = n_bins if noncoh else M                           # bins (noncoh) or windows (reference rule) per run
    if path == "direct":
        prn_chunk, runs = MAX_ROWS // rows, 1
    elif rows <= CHUNK_ROWS:
        prn_chunk, runs = CHUNK_ROWS // rows, 1
    else:
        total, other = (n_bins, M) if noncoh else (M, n_bins)
        per = max(1, CHUNK_ROWS // other)
        prn_chunk, runs = 1, -(-total // per)
    prn_chunk = min(max(prn_chunk, 1), 32)
    return dict(T=T, M=M, step=float(step), f0=f0, freqs=freqs, n_bins=n_bins, n_phi=n_phi, path=path,
                prn_chunk=prn_chunk, bin_runs=runs, per_run=per, phi_index=phi_index, shift=shift, noncoh=bool(noncoh))


def fold(s, x, g):
    """Folded windows F[w][k][n] (include/sgx.h): the carrier runs on across a window and restarts at each window."""
    N = s.samplesPerCode
    ts = 1.0 / s.samplingFreq
    n = np.arange(N)
    out = np.zeros((g["M"], g["n_bins"], N), dtype=np.complex128)
    for w in range(g["M"]):
        for k, f in enumerate(g["freqs"]):
            re = np.zeros(N)
            im = np.zeros(N)
            for m in range(g["T"]):
                blk = x[(w * g["T"] + m) * N:(w * g["T"] + m + 1) * N]
                th = f * (((n + m * N) * 2) * np.pi * ts)
                re = re + np.sin(th) * blk
                im = im + np.cos(th) * blk
            out[w, k] = re + 1j * im
    return out


def fine_window(s, g, k):
    """[lo, hi) of the 2^k-point spectrum the fine arg-max searches for a detection in bin k (T_c > 1): the indices i,
    frequency i fs / npts, within one bin step of the bin's frequency, inside the reference's [4, uniq - 5)."""
    N = s.samplesPerCode
    npts = int(8 * 2 ** (np.ceil(np.log2(10 * N))))
    uniq = int(np.ceil((npts + 1) / 2.0))
    fk = g["f0"] + g["step"] * k
    lo = int(np.ceil(((fk - g["step"]) * float(npts)) / s.samplingFreq))
    hi = int(np.floor(((fk + g["step"]) * float(npts)) / s.samplingFreq)) + 1
    lo = max(lo, 4)
    hi = min(hi, uniq - 5)
    if hi <= lo:
        hi = lo + 1
    return lo, hi


def _top2(v, offset=0):
    """((largest, its index), (second largest, its index)) of a 1-D array; indices shifted by `offset`."""
    v = np.asarray(v)
    if v.size < 2:
        return (float(v[0]), offset), (0.0, -1)
    i1 = int(v.argmax())
    w = v.copy()
    w[i1] = -np.inf
    i2 = int(w.argmax())
    return (float(v[i1]), i1 + offset), (float(v[i2]), i2 + offset)


def rel_gap(pair):
    """1 - runner-up / winner of a _top2 pair: how far the arg-max is from a tie."""
    (a, _), (b, _) = pair
    return 1.0 - b / a if a > 0 else 0.0


def coarse(s, spectra, g, code_fd):
    """One PRN's search grid res[bin, sample] from the folded windows' spectra, and the window kept per bin (reference
    rule; None for non-coherent sums)."""
    N = s.samplesPerCode
    res = np.zeros((g["n_bins"], N))
    kept = None if g["noncoh"] else np.zeros(g["n_bins"], dtype=np.int64)
    for k in range(g["n_bins"]):
        pw = [abs(np.fft.ifft(spectra[w, k] * code_fd)) ** 2 for w in range(g["M"])]
        if g["noncoh"]:
            acc = pw[0]
            for q in pw[1:]:
                acc = acc + q
            res[k] = acc
        else:
            best = 0                                    # later window wins ties (oracle.acquire's rule)
            for w in range(1, g["M"]):
                if not (pw[best].max() > pw[w].max()):
                    best = w
            res[k] = pw[best]
            kept[k] = best
    return res, kept


def fine_search(s, g, sig0dc, p, c, fbi):
    """Fine carrier arg-max of PRN index p detected at code phase c in bin fbi (acquisition.py:168-193; for T_c > 1 inside
    fine_window).  Returns (index in the reference's [4:uniq-5] slice, its frequency, the two largest magnitudes searched
    with their spectrum indices)."""
    N = s.samplesPerCode
    ts = 1.0 / s.samplingFreq
    code = orc.generate_ca_code(p)
    cvi = np.floor(ts * np.arange(1, 10 * N + 1) / (1.0 / s.codeFreqBasis))
    long_code = code[(cvi % 1023).astype(np.int64)]
    xc = sig0dc[c:c + 10 * N] * long_code
    npts = int(8 * 2 ** (np.ceil(np.log2(len(xc)))))
    mag = np.abs(np.fft.fft(xc, npts))
    uniq = int(np.ceil((npts + 1) / 2.0))
    if g["T"] > 1:
        lo, hi = fine_window(s, g, fbi)
        m = lo - 4 + int(mag[lo:hi].argmax())       # index inside the reference's [4:uniq-5] slice
    else:
        lo, hi = 4, uniq - 5
        m = int(mag[4:uniq - 5].argmax())
    return m, (np.arange(uniq) * s.samplingFreq / npts)[m], _top2(mag[lo:hi], lo)


def acquire(s, long_signal, coherent_ms=1, n_windows=2, noncoh=False, bin_step_hz=None, prn_indices=None, details=False):
    """The search, with the reference's outputs plus freqBin / fineIdx (as oracle.acquire).  IndexError where the
    reference raises it (acquisition.py:152-162).  details=True adds out["details"][p] per searched PRN index: what decides
    each arg-max and how far it is from a tie (bins, samples, fine: _top2 pairs; window: the window kept per bin)."""
    g = grid(s, coherent_ms, n_windows, noncoh, bin_step_hz)
    x = np.asarray(long_signal)
    N = s.samplesPerCode
    if x.size < g["T"] * g["M"] * N:
        raise ValueError("record too short")
    sig0dc = x - x.mean()                                   # acquisition.py:59
    spec = np.fft.fft(fold(s, x.astype(np.float64), g), axis=-1)
    table = orc.make_ca_table(s)
    spc = int(round(s.samplingFreq / s.codeFreqBasis))
    carr, cph, metric = np.zeros(32), np.zeros(32), np.zeros(32)
    fbin = np.full(32, -1, dtype=np.int64)
    fine = np.full(32, -1, dtype=np.int64)
    det = {}
    for p in (range(len(s.acqSatelliteList)) if prn_indices is None else prn_indices):
        res, kept = coarse(s, spec, g, np.fft.fft(table[p]).conj())
        fbi = int(res.max(1).argmax())
        peak = res.max(0).max()
        c = int(res.max(0).argmax())
        second = res[fbi, orc.exclusion_index(c, N, spc)].max()
        metric[p] = peak / second
        fbin[p] = fbi
        if details:
            # samples: the winning row's two largest values (the global peak lies in it) and, over all rows, the largest
            # value at any other sample - whichever runner-up is larger
            row2 = _top2(res[fbi])
            col2 = _top2(res.max(0))
            det[p] = dict(bins=_top2(res.max(1)), samples=row2 if row2[1][0] >= col2[1][0] else col2, window=kept,
                          fine=None)
        if peak / second > s.acqThreshold:
            m, f, top = fine_search(s, g, sig0dc, p, c, fbi)
            carr[p] = f
            cph[p] = c
            fine[p] = m
            if details:
                det[p]["fine"] = top
    out = dict(carrFreq=carr, codePhase=cph, peakMetric=metric, freqBin=fbin, fineIdx=fine)
    if details:
        out["details"] = det
    return out
