"""What the six record front-end stages share on the host (csrc/sgx_stage.h; DESIGN.md section 4.11, "The stage tail"):
sgx_if_filter, sgx_if_from_iq, sgx_requant_stats_of, sgx_if_requantize, sgx_cond_block_stats, sgx_if_condition.  Their
timing slots are one table and their counters are cleared by one piece of code, so: a stage writes its own slot and no
other, a record without work leaves a zero slot and zero counters and still makes a record, and a call's counters do not
carry over into the next one.  What the stages compute is the business of their own test files.

Records are two tiles plus five bytes (elements, frames) of the stage, as its *_tile() reports it; the notch has the
converter's tile, and the converter takes one byte more, because an I/Q record holds whole pairs.

The decimator, the resampler and the combiner count their clipped outputs in ONE area of the context (csrc/sgx_fir_dot4.h:
fir_run_counted), so the last test runs them one after the other on one context and holds every count and every byte
against the stage's spec.  Run with -m gpu."""
import numpy as np
import pytest

import array_spec
import decim_spec
import resamp_spec
from conftest import pkg

pytestmark = pytest.mark.gpu

STAGES = ("filter", "iq", "requant_stats", "requantize", "cond_stats", "condition")
MAKES_RECORD = ("filter", "iq", "requantize", "condition")
BLOCK = 256                       # frames per block of the conditioning stage
THETA = (16 * 50) ** 2            # the plan blanks the frames with |x| > 50 ...
PLAN_ENTRY = (0, 0, 32767, 0, THETA)   # ... and its gain of 32767 / 16 puts every other non-zero sample on a rail


@pytest.fixture(scope="module")
def ctx():
    m = pkg()
    return m.engine.get_context(m.Settings(), 0)


def lengths():
    n = pkg()._native
    return {"fir": 2 * n.iq_tile() + 5, "iq": 2 * n.iq_tile() + 6, "requant": 2 * n.requant_tile() + 5,
            "cond": 2 * n.cond_tile() + 5}


def inputs(kind):
    """The host arrays of the four stage families: "loud" clips and blanks, "zeros" cannot, "empty" has no work."""
    ln = lengths() if kind != "empty" else dict.fromkeys(("fir", "iq", "requant", "cond"), 0)
    rng = np.random.default_rng(7)
    def make(n, dtype):
        return rng.integers(-100, 101, n).astype(dtype) if kind == "loud" else np.zeros(n, dtype=dtype)
    return {"fir": make(ln["fir"], np.int8), "iq": make(ln["iq"], np.int8), "requant": make(ln["requant"], "<i2"),
            "cond": make(ln["cond"], "<i2")}


def cond_plan(frames):
    n = pkg()._native
    return np.array([PLAN_ENTRY] * (-(-frames // BLOCK)), dtype=n.COND_PLAN_DTYPE)


def run(ctx, stage, x):
    """One call of `stage` on its array of x.  Returns what the stage returned (a Record is the caller's to free)."""
    n = pkg()._native
    key = {"filter": "fir", "iq": "iq", "requant_stats": "requant", "requantize": "requant", "cond_stats": "cond",
           "condition": "cond"}[stage]
    rec = ctx.upload(np.frombuffer(np.ascontiguousarray(x[key]).tobytes(), dtype=np.int8))   # (an empty one too)
    try:
        if stage == "filter":
            return ctx.filter_record(rec, np.array([1, 2, 1], dtype=np.int16), 2)
        if stage == "iq":
            return ctx.iq_to_if(rec, *n.iq_design(15))
        if stage == "requant_stats":
            return ctx.requant_stats(rec, np.int16)
        if stage == "requantize":
            return ctx.requantize(rec, np.int16, mult=32767, shift=0)
        if stage == "cond_stats":
            return ctx.cond_stats(rec, np.int16, 1, BLOCK, 256)
        return ctx.condition(rec, np.int16, 1, BLOCK, cond_plan(x[key].size), 0)
    finally:
        rec.free()


def run_and_free(ctx, stage, x):
    out = run(ctx, stage, x)
    if stage in MAKES_RECORD:
        out.free()


def slots(ctx):
    """The six timing slots in the order of STAGES, as the float32 bits the library holds."""
    t = (ctx.filter_timing(), ctx.iq_timing()) + tuple(ctx.requant_timing()) + tuple(ctx.cond_timing())
    return np.array(t, dtype=np.float32)


def others_unchanged(before, after, i):
    keep = np.arange(len(STAGES)) != i
    assert before[keep].tobytes() == after[keep].tobytes(), (STAGES[i], before, after)


@pytest.fixture(scope="module")
def warm(ctx):
    """Every stage has run once on a record with work: all six slots hold a time."""
    x = inputs("loud")
    for stage in STAGES:
        run_and_free(ctx, stage, x)
    t = slots(ctx)
    assert np.all(t > 0.0), t
    return x


@pytest.mark.parametrize("stage", STAGES)
def test_a_stage_writes_its_own_slot_and_no_other(ctx, warm, stage):
    i = STAGES.index(stage)
    before = slots(ctx)
    assert np.all(before > 0.0), before
    run_and_free(ctx, stage, warm)
    after = slots(ctx)
    assert after[i] > 0.0, (stage, after)
    others_unchanged(before, after, i)


@pytest.mark.parametrize("stage", STAGES)
def test_a_record_without_work(ctx, warm, stage):
    i = STAGES.index(stage)
    run_and_free(ctx, stage, warm)              # the slot holds a time, the counters of the stage are not zero
    before = slots(ctx)
    assert before[i] > 0.0
    out = run(ctx, stage, inputs("empty"))
    after = slots(ctx)
    assert after[i].tobytes() == np.float32(0.0).tobytes(), (stage, after)
    others_unchanged(before, after, i)
    if stage == "requant_stats":
        assert out == dict(n_finite=0, n_nonfinite=0, max_abs=0.0, sum=0.0, sum_sq=0.0), out
    elif stage == "cond_stats":
        assert out.shape == (0,) and out.dtype == pkg()._native.COND_STATS_DTYPE
    else:
        assert len(out) == 0
        assert getattr(out, "clipped", 0) == 0 and getattr(out, "blanked", 0) == 0
        assert (stage == "condition") == hasattr(out, "blanked") and (stage in ("requantize", "condition")) == hasattr(out, "clipped")
        out.free()
        assert not out._h
        out.free()                              # (a second free is harmless)


@pytest.mark.parametrize("stage", ["requantize", "condition"])
def test_counters_start_from_zero_on_every_call(ctx, stage):
    loud = run(ctx, stage, inputs("loud"))
    quiet = run(ctx, stage, inputs("zeros"))
    try:
        x = inputs("loud")["requant" if stage == "requantize" else "cond"]
        if stage == "requantize":
            assert loud.clipped == np.count_nonzero(x) > 0
        else:
            hit = np.abs(x.astype(np.int64)) > 50
            assert loud.blanked == np.count_nonzero(hit) > 0
            assert loud.clipped == np.count_nonzero((x != 0) & ~hit) > 0
            assert quiet.blanked == 0
        assert quiet.clipped == 0
        assert len(quiet) == len(loud) == x.size and not quiet.download().any()
    finally:
        loud.free()
        quiet.free()


def clip_area_cases():
    """(name, input bytes, call on a context and a record, (spec bytes, spec count)) of the stages that share the clip area:
    a decimation (D = 3, I/Q) and a combine (A = 3, I/Q) of loud records through taps that must clip, and a resampling (L / M
    = 3 / 2) of a quiet record through small taps that cannot: at most 9 taps of a stream meet a sample, 9 x 64 x 20 >> 8 is
    45.  Outputs are three tiles of the stage plus 17 bytes - a workgroup with a whole tile, a seam, a whole 16-byte store
    and byte stores behind the last tile, four counter slots -, and one byte more where the record is I/Q, whose outputs
    are whole pairs."""
    n = pkg()._native
    rng = np.random.default_rng(11)
    n_dec, n_res, n_com = 3 * n.decim_tile() + 18, 3 * n.resamp_tile() + 17, 3 * n.combine_tile() + 18
    x_dec = rng.integers(-100, 101, 2 * (3 * (n_dec // 2) - 1)).astype(np.int8)      # ceil(frames / 3) = n_dec / 2
    h_dec = rng.integers(-2000, 2001, 2 * 9).astype(np.int16)
    x_res = rng.integers(-20, 21, (2 * n_res) // 3).astype(np.int8)                   # ceil(3 N / 2) = n_res
    h_res = np.full(25, 64, dtype=np.int16)
    x_com = rng.integers(-100, 101, 3 * n_com).astype(np.int8)
    h_com = rng.integers(-3000, 3001, (3, 3, 2)).astype(np.int16)
    cases = [("decimate", x_dec, lambda c, r: c.decimate(r, 2, h_dec, 6, 3), decim_spec.decimate(x_dec, h_dec, 6, 2, 3)),
             ("resample", x_res, lambda c, r: c.resample(r, h_res, 8, 3, 2), resamp_spec.resample(x_res, h_res, 8, 3, 2)),
             ("combine", x_com, lambda c, r: c.combine(r, 2, 3, h_com, 6), array_spec.combine(x_com, h_com, 6, 2, 3))]
    for (name, _, _, (y, count)), size in zip(cases, (n_dec, n_res, n_com)):
        assert y.size == size, (name, y.size, size)
        assert (count == 0) == (name == "resample"), (name, count)       # the specs alone: (a) and (c) clip, (b) never does
    return cases


def test_the_fir_stages_share_one_clip_area_and_each_count_is_its_own(ctx):
    dec, res, com = clip_area_cases()
    for name, x, call, (want, count) in (dec, res, com, res):
        rec = ctx.upload(x)
        try:
            out = call(ctx, rec)
        finally:
            rec.free()
        try:
            print(name, "clipped", out.clipped, "spec", count)
            assert out.clipped == count, (name, out.clipped, count)
            assert out.download().tobytes() == want.tobytes(), name
        finally:
            out.free()
