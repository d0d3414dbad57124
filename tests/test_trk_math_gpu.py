"""The arithmetic of the tracking chain as the DEVICE compiles it (sgx_trk_math_eval_device, csrc/sgx_trk_math_dev.hip):
csrc/sgx_trk_math.h through the fn -> call table the host evaluator runs too, and div_rn, sincos_turns, ramp_setup and
prep_code of csrc/sgx_trk_common.h.  What must be EQUAL (the divisions that feed integer roundings, block lengths, chip
switches, prep_code's outputs) is compared with numpy's IEEE fp64 without a tolerance; what may differ by a few ulp is bounded
against 50-digit arithmetic by the bounds tests/test_cabi_and_host.py asserts on the host compilation.  Operands and
references: tests/trk_math_cases.py.  Every test is a few launches of at most 2^20 elements.  Run with -m gpu."""
import numpy as np
import pytest

import trk_math_cases as tm
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    m = pkg()
    return m.engine.get_context(m.Settings(), 0)


@pytest.fixture(scope="module")
def ev(ctx):
    def evaluate(name, *operands):
        return pkg()._native.trk_math_eval(tm.FN[name], *operands, ctx=ctx)
    return evaluate


# ---- equalities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copy", ["div_rn", "sgx_div_rn"])
def test_reciprocal_division_equals_ieee_division(ev, copy):
    """div_rn (csrc/sgx_trk_common.h) and sgx_div_rn (csrc/sgx_trk_math.h) == a / b for b = pi, every sampling rate (a: code
    frequencies within 60 Hz of the basis, and every block length within 60 of fs / 1000: the PLL waves' blk / fs) and the
    eight block lengths of every rate (a: 1023 +- 2e-3, and the spans prep_code forms); y = 1.0 / b as the host forms it"""
    classes = tm.div_rn_operands()
    assert classes["blk_over_fs"][0].size == 13 * 121 and sum(a.size for a, _ in classes.values()) <= 1 << 20
    names = sorted(classes)
    a = np.concatenate([classes[k][0] for k in names])
    b = np.concatenate([classes[k][1] for k in names])
    which = np.concatenate([np.full(classes[k][0].size, j) for j, k in enumerate(names)])
    got = ev(copy, a, b, 1.0 / b)[0]
    assert not (msg := tm.first_mismatch(got, a / b, a=a, b=b, divisor_class=which)), (names, msg)


def test_block_length_equals_the_reference(ev):
    """sgx_block_length(a, cf, fs) == ceil(a / (cf / fs)), step_a within 3 ulp of cf / fs, and both outputs of the second
    entry agree with the first; a quarter of the quotients at or a few numbers next to an integer, block 0 of every rate"""
    a, cf, fs = tm.block_length_operands(40000, 178)
    assert a.size <= 1 << 20
    step = cf / fs
    blk, step_a = ev("block_length", a, cf, fs, 1.0 / fs)
    assert not (msg := tm.first_mismatch(blk, np.ceil(a / step), a=a, codeFreq=cf, fs=fs)), msg
    bad = np.flatnonzero(~(np.abs(step_a - step) <= 3 * np.spacing(step)))
    assert bad.size == 0, (float(cf[bad[0]]), float(fs[bad[0]]), float(step_a[bad[0]]), float(step[bad[0]]))
    blk2, inv_step = ev("block_length_inv", a, cf, fs, 1.0 / fs)
    assert np.array_equal(blk, blk2)
    # "~1 / step_a (2^-40)": one Newton step on a seed of at least 20 bits
    assert np.all(np.abs(inv_step * step_a - 1.0) <= 2.0 ** -40)
    first = np.flatnonzero(np.r_[True, fs[1:] != fs[:-1]])
    assert np.all(a[first] == 1023.0) and np.all(cf[first] == 1.023e6) and first.size == 13


def test_division_free_ceil_equals_ieee_ceil(ev):
    """sgx_ceil_div(a, step) == ceil(a / step) on the same operands (prep_code's block length)"""
    a, cf, fs = tm.block_length_operands(40000, 108)
    step = cf / fs
    got = ev("ceil_div", a, step)[0]
    assert not (msg := tm.first_mismatch(got, np.ceil(a / step), a=a, step=step, fs=fs)), msg


def test_ramp_setup_equals_brute_force(ev):
    """ramp_setup == (ceil(t(ilo)), the first i with t(i) > it) searched sample by sample, t(i) = float64(i) * step + start,
    on the E / P / L ramps of every rate (the two with about four samples per chip too) and spacing; for at least a quarter
    the start is such that a t(i) near the switch is an integer or within 4 ulp of one"""
    start, step, code_step, ilo, fs, near = tm.ramp_operands(1500, 31)
    assert start.size <= 1 << 20 and near.mean() >= 0.25
    k1, isw = ev("ramp_setup", start, step, code_step, ilo)
    want_k1, want_isw = tm.ramp_reference(start, step, ilo, fs)
    # the moved starts do what they are for: at a quarter of ALL cases the sample at the switch, or the one before it, has
    # t(i) on the integer k1 or within 4 ulp of it
    t_sw = want_isw * step + start
    t_before = (want_isw - 1.0) * step + start
    close = np.minimum(np.abs(t_sw - want_k1), np.abs(t_before - want_k1)) <= 4 * np.spacing(np.maximum(want_k1, 1.0))
    assert close.mean() >= 0.25, close.mean()
    assert not (msg := tm.first_mismatch(k1, want_k1, start=start, step=step, ilo=ilo, fs=fs)), msg
    assert not (msg := tm.first_mismatch(isw, want_isw, start=start, step=step, ilo=ilo, fs=fs, code_step=code_step)), msg


@pytest.mark.parametrize("spacing", tm.SPACINGS)
def test_prep_code_equals_the_reference(ev, spacing):
    """prep_code == tracking.py:148-190 restated in numpy (tests/trk_math_cases.py: prep_reference, which
    tests/test_trk_math_host.py holds against the oracle's np.linspace ramps), every output bit for bit: blk, the three
    steps, the three starts, remCode - for block lengths among the eight precomputed reciprocals and outside them"""
    for k, fs in enumerate(tm.FS):
        cf, rem = tm.prep_operands(fs, 8000, 500 + k)
        r = tm.prep_reference(cf, rem, fs, spacing)
        known = (r["blk"] >= tm.nb_base(fs)) & (r["blk"] < tm.nb_base(fs) + 8)
        assert known.sum() >= 1000 and (~known).sum() >= 1000, (fs, known.sum())
        f, s = np.full(cf.size, fs), np.full(cf.size, spacing)
        what = dict(codeFreq=cf, rem=rem, fs=f)
        blk, rem_code = ev("prep_blk", cf, rem, f, s)
        assert not (msg := tm.first_mismatch(blk, r["blk"], **what)), msg
        assert not (msg := tm.first_mismatch(rem_code, r["remCode"], **what)), msg
        for arm in "EPL":
            stp, start = ev("prep_" + arm, cf, rem, f, s)
            assert not (msg := tm.first_mismatch(stp, r["step" + arm], blk=blk, **what)), (arm, msg)
            assert not (msg := tm.first_mismatch(start, r["start" + arm], **what)), (arm, msg)
        inv_step, stop = ev("prep_inv", cf, rem, f, s)
        assert np.all(np.abs(inv_step * r["step"] - 1.0) <= 2.0 ** -40) and not stop.any()


# ---- ulp bounds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [("rcp", "fast_div", "div1"), ("fast_sqrt", "sqrt1", "sqrt1_pos"), ("atan_ratio",),
                                   ("atan_ratio_k",), ("sincos_turns_short", "sincos_turns"), ("rot_small",)],
                         ids=lambda n: "-".join(n))
def test_ulp_bounds(ev, names):
    """worst error over 2^18 operands per function - the host tests' distributions, envelope sums 1e2 .. 1e9 and
    (E - L) / (E + L) with E ~ L, quotients at SGX_ATAN_SHORT_MAX +- a few numbers - screened in long double, then in
    50-digit arithmetic on the 2 000 worst and 2 000 random ones.  Bounds: those of tests/test_cabi_and_host.py;
    sgx_sqrt1_pos as sgx_sqrt1, sincos_turns as its Estrin twin.  The atan's error is reported per path.  Prints the figures
    of DESIGN.md 4.1's table (-s)."""
    rep = tm.ulp_report(ev, names)
    for label in sorted(rep):
        print("device %-24s %.3f at %r" % (label, rep[label][0], rep[label][1]))
    assert set(k.split("/")[0] for k in rep) == set(names)
    bad = {k: v for k, v in rep.items() if not v[0] <= tm.bound_of(k)}
    assert not bad, bad


# ---- degenerate values ---------------------------------------------------------------------------------------------------------
def test_degenerate_values(ev):
    """a silent record's arithmetic: sgx_sqrt1(0) == 0, sgx_sqrt1_pos(0) and sgx_div1(0, 0) are NaN, the atan's follow numpy's
    arctan(q / i) through zeros, infinities and NaN"""
    z = np.zeros(1)
    assert ev("sqrt1", z)[0][0] == 0.0 and ev("fast_sqrt", z)[0][0] == 0.0
    assert np.isnan(ev("sqrt1_pos", z)[0][0])
    assert np.isnan(ev("div1", z, z)[0][0])
    vals = [0.0, -0.0, 1.0, -1.0, 0.2, 3.0, np.inf, -np.inf, np.nan]
    q = np.array([x for x in vals for _ in vals])
    i = np.array([y for _ in vals for y in vals])
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.arctan(q / i)
    for name in ("atan_ratio", "atan_ratio_k"):
        got = ev(name, q, i)[0]
        one = ev(name, np.array([1.0, -1.0, 0.0]), np.zeros(3))[0]
        assert one[0] == np.arctan(np.inf) and one[1] == -np.arctan(np.inf) and np.isnan(one[2]), (name, one)
        special = ~np.isfinite(q) | ~np.isfinite(i) | (i == 0)
        same = (got == want) | (np.isnan(got) & np.isnan(want))
        assert same[special].all(), (name, q[special & ~same], i[special & ~same], got[special & ~same])


def test_block_length_of_a_degenerate_code_frequency_stops_the_kernels(ev):
    """codeFreq NaN, +-inf, 0 or negative (what a silent record's NaN discriminator makes of the NCO): the block length
    sgx_block_length returns lies outside [1, lim], lim = the longest block any launch provides - the kernels' stop test
    (unsigned)(blk - 1) >= lim then ends the channel"""
    cf = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.023e6, -1.0, -1e-300, -1e300])
    a = np.array([1023.0, 1022.99, 1023.01, np.nan])
    for fs in tm.FS:
        aa, cc = np.repeat(a, cf.size), np.tile(cf, a.size)
        f = np.full(aa.size, fs)
        blk = ev("block_length", aa, cc, f, 1.0 / f)[0]
        inside = (blk >= 1) & (blk <= tm.LIM)
        assert not inside.any(), (fs, aa[inside], cc[inside], blk[inside])


def test_a_degenerate_step_stops_prep_code(ev):
    """the same for the kernels that go through prep_code (throughput, multi, per-sample, float, any-type): sgx_ceil_div of a
    NaN, infinite, zero or negative step is no length 1 .. LIM, and prep_code posts stop = 1 for every such code frequency -
    tested on the step itself, whatever the device's float -> int conversion makes of a NaN quotient"""
    step = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.023e6 / 38.192e6, -1e-300, 1e-300])
    for a in (1023.0, 1022.99, np.nan):
        blk = ev("ceil_div", np.full(step.size, a), step)[0]
        assert not np.any((blk >= 1) & (blk <= tm.LIM)), (a, blk)
    cf = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.023e6, -1.0, -1e-300, -1e300, 1.023e6])
    rem = np.array([0.0, 0.01])
    for fs in tm.FS:
        cc, rr = np.tile(cf, rem.size), np.repeat(rem, cf.size)
        f, s = np.full(cc.size, fs), np.full(cc.size, 0.5)
        stop = ev("prep_inv", cc, rr, f, s)[1]
        sound = cc == 1.023e6                          # (the one code frequency of the list that has a block)
        assert np.all(stop[~sound] == 1.0) and np.all(stop[sound] == 0.0), (fs, cc, rr, stop)
