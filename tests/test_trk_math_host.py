"""The arithmetic of the tracking chain as the HOST compiles it (sgx_trk_math_eval_batch: the fn -> call table of
csrc/sgx_trk_math_eval.h with float-precision seeds and glibc's atan), on the operands of tests/trk_math_cases.py, and
that module's own references against the oracle.  tests/test_trk_math_gpu.py runs the same table on the device."""
import importlib

import numpy as np
import pytest

import trk_math_cases as tm
from conftest import pkg
from oracle import softgnss_oracle as orc


@pytest.fixture(scope="module")
def built():
    importlib.import_module("__graft_entry__").build()
    return pkg()


def ev(name, *operands):
    if tm.FN[name] >= 16:
        raise NotImplementedError(name)
    return pkg()._native.trk_math_eval(tm.FN[name], *operands)


def test_the_rates_are_the_ones_the_suite_tracks_at():
    import any_rate
    assert len(tm.FS) == 13 == len(set(tm.FS))
    assert sorted(tm.n_code(f) for f in tm.FS) == sorted(any_rate.SMOOTH_IN_USE + [int(round(f / 1000)) for f, _ in any_rate.RATES])
    assert set(f for f, _ in any_rate.RATES) <= set(tm.FS)


def test_block_reference_is_the_oracles():
    """prep_reference (the elementwise restatement the prep_code tests compare with) against the oracle's own np.linspace
    ramps and its code-phase update, bit for bit, at every rate and spacing"""
    for k, fs in enumerate(tm.FS):
        for spc in tm.SPACINGS:
            s = orc.OracleSettings(samplingFreq=fs, IF=fs / 4, dllCorrelatorSpacing=spc)
            cf, rem = tm.prep_operands(fs, 12, 1000 + k)
            r = tm.prep_reference(cf, rem, fs, spc)
            for j in range(cf.size):
                step = cf[j] / s.samplingFreq
                blk = int(np.ceil((s.codeLength - rem[j]) / step))
                assert blk == r["blk"][j] and step == r["step"][j]
                for arm, off in (("E", -spc), ("P", 0.0), ("L", spc)):      # (x - spc == x + (-spc); x + 0.0 == x)
                    t = np.linspace(rem[j] + off, blk * step + rem[j] + off, blk, endpoint=False)
                    i = np.arange(blk, dtype=np.float64)
                    assert np.array_equal(t, i * r["step" + arm][j] + r["start" + arm][j]), (fs, spc, arm, cf[j], rem[j])
                    if arm == "P":
                        assert t[blk - 1] + step - 1023.0 == r["remCode"][j]


def test_compiled_reciprocal_division_equals_ieee_division(built):
    """sgx_div_rn as compiled == a / b on every divisor class, no tolerance"""
    for name, (a, b) in tm.div_rn_operands().items():
        got = ev("sgx_div_rn", a, b, 1.0 / b)[0]
        assert not (msg := tm.first_mismatch(got, a / b, a=a, b=b)), (name, msg)


def test_ulp_bounds_on_the_batch_operands(built):
    """every function's worst error over 2^18 operands (long-double screen, 50-digit arithmetic on the worst and on random
    ones): the bounds of tests/test_cabi_and_host.py on the wider distributions the device test uses; prints the figures
    of DESIGN.md 4.1's table (-s)"""
    rep = tm.ulp_report(ev)
    for label in sorted(rep):
        print("host %-24s %.3f at %r" % (label, rep[label][0], rep[label][1]))
    bad = {k: v for k, v in rep.items() if not v[0] <= tm.bound_of(k)}
    assert not bad, bad


def test_degenerate_values(built):
    assert ev("sqrt1", [0.0])[0][0] == 0.0
    assert np.isnan(ev("sqrt1_pos", [0.0])[0][0]) and np.isnan(ev("div1", [0.0], [0.0])[0][0])
    cf = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.023e6, -1.0])
    for fs in tm.FS:
        f = np.full(cf.size, fs)
        blk = ev("block_length", np.full(cf.size, 1023.0), cf, f, 1.0 / f)[0]
        assert not np.any((blk >= 1) & (blk <= tm.LIM)), (fs, blk)


def test_division_free_ceil_of_a_degenerate_step(built):
    """sgx_ceil_div(a, step) with the step a NaN, infinite, zero or negative code frequency leaves (prep_code's block length
    on a silent record): never a length a launch could run, 1 .. LIM"""
    step = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.023e6 / 38.192e6, -1e-300, 1e-300])
    for a in (1023.0, 1022.99, np.nan):
        blk = ev("ceil_div", np.full(step.size, a), step)[0]
        assert not np.any((blk >= 1) & (blk <= tm.LIM)), (a, blk)
