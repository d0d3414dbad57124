"""The radix-pass kernels of csrc/sgx_fft.hip (fft_pass_kernel<R, TPB, MODE>) on the GPU, at every length of
tests/fft_cover.py: every radix as first, middle and last pass, plain and fused, on lengths that factor and on padded ones.
The transforms themselves against numpy's FFT on long double (80-bit extended: complex256) through sgx_fft_run_passes, to a
bound derived from the plan (fft_cover.error_bound); then acquisition against oracle.acquire at every length, to the bars
of tests/test_any_rate_gpu.py, with a detection in every output slot of the last radix.  tests/test_fft_cover_host.py
asserts the table's coverage and conditions every scene in numpy.  Last, whose tables a transform reads: a plan's own
(sgx_fft_plan_create), through contexts that close, lengths that alternate and a context's first call.  Run with -m gpu."""
import numpy as np
import pytest

import fft_cover as fc
from conftest import load_golden, pkg
from oracle import softgnss_oracle as orc
from test_any_rate_gpu import _same_search
from test_gpu_parity import check_acq_default_golden

pytestmark = pytest.mark.gpu


def _ctx():
    m = pkg()
    return m.engine.get_context(m.Settings(), 0)


@pytest.mark.parametrize("n", fc.LENGTHS)
def test_plain_transform_against_long_double(n):
    """sgx_fft_forward on random rows, zero-tailed rows (nonzero_len = 1, n / R1 - 1, n / R1 + 1, n - 1), a unit impulse in
    every residue class of the first radix and a pure tone per pass, several rows per call; row by row
    ||X^ - X||_2 / ||X||_2 against numpy.fft.fft on clongdouble.

    The bound is fft_cover.error_bound(radices), derived there from the passes sgx_acquire_fft_passes reports and not
    from what the kernels give: (R + 1 + sqrt(8)) u per butterfly plus (2 + 2 sqrt(8)) u per twiddled pass, summed over
    the passes, u = 2^-53: 1.3e-14 for 131 072 = 16^4 2 and for 29 791 = 31^3, 7.4e-15 for 2 048.  A wrong root or twiddle entry
    gives an error near 1, a float-precision constant about 1e-8.  numpy's float64 FFT against the same long-double
    result is printed next to it: the reference's own arithmetic (one "FFTERR" line per length, with the kernels'
    figure and the bound)."""
    c = fc.plan(n)
    ctx = _ctx()
    bound = fc.error_bound(c.radices)
    worst, worst_np = 0.0, 0.0
    for name, rows, t in fc.plain_rows(c, 0xF0F7 + n):
        got = ctx.fft_forward(rows, t)
        cut = rows.copy()
        cut[:, t:] = 0.0
        want = fc.fft_long(cut)
        err, err_np = fc.rel_err(got, want), fc.rel_err(np.fft.fft(cut, axis=-1), want)
        print("%d %s: kernel %.2e, numpy float64 %.2e, bound %.2e" % (n, name, err.max(), err_np.max(), bound))
        worst, worst_np = max(worst, err.max()), max(worst_np, err_np.max())
        assert np.all(err <= bound), (name, err, bound)
        if name == "tone":
            # exactly one output is nonzero: everything else is rounding, far below one part in 10^12 of it
            for r in range(rows.shape[0]):
                k = int(np.argmax(np.abs(want[r])))
                rest = np.delete(np.abs(got[r]), k)
                assert abs(got[r, k]) > 0.5 * c.length and rest.max() <= 1e-12 * c.length, (r, k, rest.max())
    print("FFTERR %d %s kernel %.3e numpy64 %.3e bound %.3e" % (n, "x".join(map(str, c.radices)), worst, worst_np, bound))


def _check_peaks(c, mx, arg, x_rows, f_rows, n_valid, what):
    want_mx, want_arg, ref = fc.fused_reference(x_rows, f_rows, n_valid)
    assert np.array_equal(arg, want_arg), (what, arg, want_arg)
    # |y^_k - y_k| <= bound ||y||_2 (normwise), the power is its square scaled by an exact-to-1-u 1/n: 2 bound ||y|| / |y_k|
    # plus 4 u for the scale, the two squares and their sum
    bound = fc.error_bound(c.radices, fused_first=True)
    norm = np.sqrt(np.sum(np.abs(ref) ** 2, axis=-1)).astype(np.float64)
    peak = np.abs(ref[np.arange(len(want_arg)), want_arg]).astype(np.float64)
    tol = 2.0 * bound * norm / peak + 4.0 * fc.U
    rel = np.abs(mx / want_mx - 1.0)
    print("%d %s: max relative error of the peak power %.2e (allowed %.2e)" % (c.n, what, rel.max(), tol.min()))
    assert np.all(rel <= tol), (what, rel, tol)


@pytest.mark.parametrize("n", fc.LENGTHS)
def test_fused_correlation_against_long_double(n):
    """MODE 1 into MODE 2 (a length that factors) or MODE 3 (a padded one) and acq_rowmax_finish_kernel: rows built
    backwards from the wanted output (mul_x = conj(ifft(y)), mul_f = 1 and -i), the dominant value at every slot q of the
    last radix, in the first and last workgroup, lanes 0 and TPB - 1, the partial last workgroup, n_valid - 1; at n_valid
    and deep in the discarded tail a still larger value that must not win.  arg exactly, max to the derived bound; once
    with rows_per_prn > 1 and once with a row map; the row map again into MODE 0 (the second-peak route) against the
    long-double rows; an impulse at 0 makes every output 1 bit for bit, and the answer must be index 0."""
    c = fc.plan(n)
    ctx = _ctx()
    L = c.length
    n_valid = c.n if c.padded else 0
    names, idx = zip(*fc.dominant_indices(c))
    idx, also = list(idx), []
    if c.padded:
        also = [(len(idx), c.n), (len(idx) + 1, L - 3), (len(idx) + 2, c.n + (L - c.n) // 2)]
        idx += [idx[0], c.n - 1, c.n // 2]
    K = len(idx)
    x, _ = fc.backwards_rows(c, idx, 0xB0C5 + n, also=also)
    f = np.stack([np.ones(L, dtype=np.complex128), -1j * np.ones(L, dtype=np.complex128)])
    # regular layout: row r = (r % K, r // K)
    mx, arg = ctx.fft_fused(x, f, 2 * K, rows_per_prn=K, n_valid=n_valid)
    rb, rp = np.arange(2 * K) % K, np.arange(2 * K) // K
    _check_peaks(c, mx, arg, x[rb], f[rp], n_valid or L, "regular")
    for r in range(2 * K):      # (a slot of a padded length may lie wholly at or above n_valid: then it must not win)
        assert (arg[r] == idx[r % K]) == (idx[r % K] < (n_valid or L)), (r, arg[r], idx[r % K])
    # row map
    rmap = np.array([(K - 1 - r, r % 2) for r in range(K)], dtype=np.int32)
    mx, arg = ctx.fft_fused(x, f, K, row_map=rmap, n_valid=n_valid)
    _check_peaks(c, mx, arg, x[rmap[:, 0]], f[rmap[:, 1]], n_valid or L, "row map")
    # the rows themselves: MODE 1 into MODE 0
    rows = ctx.fft_fused(x, f, K, row_map=rmap, want_rows=True)
    want = fc.fused_reference(x[rmap[:, 0]], f[rmap[:, 1]], L)[2]
    err = fc.rel_err(rows, want)
    assert np.all(err <= fc.error_bound(c.radices, fused_first=True)), err
    # the tie rule: an impulse at 0 against ones gives 1 + 0i everywhere, exactly
    e0 = np.zeros((1, L), dtype=np.complex128)
    e0[0, 0] = 1.0
    one = (1.0 / L) * (1.0 / L)
    for nv in {0, c.n if c.padded else L - 1}:
        mx, arg = ctx.fft_fused(e0, f[:1], 1, n_valid=nv)
        assert arg[0] == 0 and mx[0] == one, (nv, arg, mx, one)


def test_hook_refuses_what_the_plan_refuses():
    m = pkg()
    ctx = _ctx()
    with pytest.raises(m._native.SgxError, match="prime factor above 31"):
        ctx.fft_forward(np.ones((1, 4099), dtype=np.complex128))
    with pytest.raises(m._native.SgxError):
        ctx.fft_fused(np.ones((1, 4096), dtype=np.complex128), np.ones((1, 4096), dtype=np.complex128), 2, rows_per_prn=1)
    with pytest.raises(m._native.SgxError, match="cannot fuse both ends"):
        ctx.fft_fused(np.ones((1, 31), dtype=np.complex128), np.ones((1, 31), dtype=np.complex128), 1)


@pytest.mark.parametrize("n", fc.LENGTHS)
def test_acquisition_against_oracle_with_a_peak_in_every_slot(n):
    """sgx_acquire at samplesPerCode n against oracle.acquire: codePhase, freqBin, fineIdx and carrFreq exactly, peakMetric
    within 1e-9; over the scenes of a length every output slot of the last radix holds one detection's code phase."""
    m = pkg()
    c = fc.plan(n)
    won = set()
    for prns, phases, x in fc.scene_records(n):
        a = m.AcquisitionResult(fc.settings(n, prns), device=0)
        a.acquire(x)
        ref = orc.acquire(fc.oracle_settings(n, prns), x)
        _same_search(a, ref, [p - 1 for p in prns])
        assert all(ref["carrFreq"][p - 1] > 0 for p in prns)
        won |= fc.winning_slots(c, ref, prns)
    assert won == set(c.slots())


def test_noncoherent_route_with_more_than_64_last_pass_workgroups():
    m = pkg()
    n = fc.NONCOH_N
    prns, phases, x = fc.scene_records(n)[0]
    a = m.AcquisitionResult(fc.settings(n, prns), device=0)
    a.acquire(x, n_blocks=4, noncoh=True)
    ref = orc.acquire(fc.oracle_settings(n, prns), x, n_blocks=4, noncoh=True)
    _same_search(a, ref, [p - 1 for p in prns])
    assert all(ref["carrFreq"][p - 1] > 0 for p in prns)


def test_deferred_and_queued_entry_with_more_than_64_last_pass_workgroups():
    m = pkg()
    n = fc.DEFERRED_N
    prns, phases, x = fc.scene_records(n)[0]
    s = fc.settings(n, prns)
    idx = [p - 1 for p in prns]
    ctx = m.engine.get_context(s, 0)
    rec = ctx.upload(x)
    try:
        want = ctx.acquire(rec, 0, 11 * n, idx)
        ctx.acquire_begin(rec, 0, 11 * n, idx)
        got = ctx.acquire_end(len(idx))
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        a = m.AcquisitionResult(s, device=0, deferred=True)
        a.acquire(m.DeviceSignal(rec, 0, 11 * n))
        _same_search(a, orc.acquire(fc.oracle_settings(n, prns), x), idx)
        assert np.sum(a.carrFreq > 0) == len(prns)
    finally:
        rec.free()


# ---- the tables belong to the plan that reads them (sgx_fft_plan_create), and so to one context or one call ----

def _random_rows(n, rows, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))


def _within_bound(got, rows, n):
    err, bound = fc.rel_err(got, fc.fft_long(rows)), fc.error_bound(fc.plan(n).radices)
    print("%d: kernel %.2e, bound %.2e" % (n, err.max(), bound))
    return np.all(err <= bound)


def test_tables_die_with_their_owner_and_with_no_one_elses():
    """Two contexts on one device, 496 = 16 x 31 on both; closing one leaves the other's transform as it was, bit for bit."""
    m = pkg()
    s = m.Settings()
    rows = _random_rows(496, 3, 0x7AB1E)
    with m.engine.private_context(s, 0) as second:
        with m.engine.private_context(s, 0) as first:
            assert first is not second
            got_first = first.fft_forward(rows)
            before = second.fft_forward(rows)
        after = second.fft_forward(rows)     # (`first` and everything it owned is gone)
    assert np.array_equal(after, before) and np.array_equal(got_first, before)
    assert _within_bound(after, rows, 496)


def test_a_plan_that_changes_length_rebuilds_all_of_its_tables():
    """210 = 2 3 5 7, 899 = 29 31, 210 again on one context: no radix, and no table, is shared between the two lengths."""
    ctx = _ctx()
    x210, x899 = _random_rows(210, 3, 0x210), _random_rows(899, 3, 0x899)
    a = ctx.fft_forward(x210)
    b = ctx.fft_forward(x899)
    c = ctx.fft_forward(x210)
    assert np.array_equal(c, a)
    assert _within_bound(a, x210, 210) and _within_bound(b, x899, 899) and _within_bound(c, x210, 210)


def test_a_search_is_the_same_after_a_transform_of_another_length(default_record):
    """The context's own plans (code length, fine search) with another length's transform between two searches."""
    ctx = _ctx()
    x = default_record[:11 * 38192].astype(np.float64)
    first = ctx.acquire_f64(x, range(32))
    ctx.fft_forward(_random_rows(899, 1, 0x899))
    again = ctx.acquire_f64(x, range(32))
    assert sorted(first) == ["carrFreq", "codePhase", "fineIdx", "freqBin", "peakMetric"]
    for k in first:
        assert np.array_equal(again[k], first[k]), k
    assert np.any(first["carrFreq"] > 0)      # (the fine search ran)


def test_four_step_and_fine_tables_on_a_fresh_context(default_record):
    """A new context's very first call is the search of all 32 PRNs (four-step and fine-search tables); twice in one
    process, each context closed before the next opens: the second finds nothing the first left behind."""
    g = load_golden("acq_default.npz")
    m = pkg()
    s = m.Settings()
    for _ in range(2):
        with m.engine.private_context(s, 0):
            a = m.AcquisitionResult(s, device=0)     # (engine.get_context hands out the thread's private context)
            a.acquire(default_record[:int(g["n_samples"])])
            check_acq_default_golden(a, g)
