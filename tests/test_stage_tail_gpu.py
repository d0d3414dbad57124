"""What the six record front-end stages share on the host (csrc/sgx_stage.h; DESIGN.md section 4.11, "The stage tail"):
sgx_if_filter, sgx_if_from_iq, sgx_requant_stats_of, sgx_if_requantize, sgx_cond_block_stats, sgx_if_condition.  Their
timing slots are one table and their counters are cleared by one piece of code, so: a stage writes its own slot and no
other, a record without work leaves a zero slot and zero counters and still makes a record, and a call's counters do not
carry over into the next one.  What the stages compute is the business of their own test files.

Records are two tiles plus five bytes (elements, frames) of the stage, as its *_tile() reports it; the notch has the
converter's tile, and the converter takes one byte more, because an I/Q record holds whole pairs.

All nine counting entry points - requantize, condition, unpack, decimate, resample, combine, combine_blocks, excise_record,
if_cancel - count in ONE area of the context (csrc/sgx_count.h, SgxStage::count), so the last test runs every one of them
behind every other on one context and holds every count and every byte against the stage's spec.  Run with -m gpu."""
import numpy as np
import pytest

import array_block_spec
import array_spec
import cancel_cases
import cancel_spec
import cond_spec
import decim_spec
import excise_cases
import excise_spec
import requant_spec
import resamp_spec
import unpack_spec
from conftest import pkg
from oracle import softgnss_oracle as orc

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


def as_bytes(x):
    return np.frombuffer(np.ascontiguousarray(x).tobytes(), dtype=np.int8)


def reads(call, *names):
    """call(context, record) -> a record, as (context, record) -> (the record, its counters `names`)"""
    def wrapped(c, r):
        out = call(c, r)
        return out, tuple(int(getattr(out, k)) for k in names)
    return wrapped


def counter_area_cases():
    """(name, input bytes, call on a context and a record -> (record, its counters), (spec bytes, spec counters)) of all
    nine counting entry points, which share ONE counter area (csrc/sgx_count.h): the three cases of clip_area_cases() as
    they stand, and one case each of the requantiser (clipped), the conditioning stage (blanked, clipped), the unpacker at
    2 and at 4 bits (4 and 16 code counts), the block combiner (clipped) and the excision (bins_cut, segments_cut, clipped)
    on outputs of three tiles plus 17 bytes (one more for I/Q; the excision: three tiles of its plan at N = 64 and a
    little of the next, excise_cases.tile_span).  Then one case per shape of the publish with more workgroups than the
    256 slots of the area, so that a slot takes the atomics of two workgroups: 257 tiles plus 17 bytes of the requantiser
    (one counter), the conditioning stage (two), the 4-bit unpacker (sixteen) and the excision (per wave).  Last the
    cancellation (clipped), whose blocks are those of hand-made channels at 2.046 Msps (cancel_cases.handmade) at ten times
    a sensible amplitude: three tiles plus 17 bytes, and 257 tiles plus 17 bytes with one channel's blocks in tile 0 and
    the other's in tile 256, both of which clip - two workgroups add into slot 0.  Expected bytes
    and counters come from the stage's spec module alone, and on those alone: every counter of every case is above zero
    but the resampling's, which is zero; the excision's cases keep excise_spec.MARGIN as tests/excise_cases.py asks; the
    cancellation's cases have no rounding decision (cancel_spec.decisions), so their bytes are compared exactly too."""
    n = pkg()._native
    rng = np.random.default_rng(11)
    cases = [(name, x, reads(call, "clipped"), (y, (count,))) for name, x, call, (y, count) in clip_area_cases()]

    def requantize(tag, tiles):
        x = rng.integers(-100, 101, tiles * n.requant_tile() + 17).astype("<i2")
        y = requant_spec.quantise(as_bytes(x), np.int16, 3, 1)                 # |x| >= 85 lands on a rail
        call = reads(lambda c, r: c.requantize(r, np.int16, mult=3, shift=1), "clipped")
        return ("requantize" + tag, as_bytes(x), call, (y, (int(np.count_nonzero(np.abs(y.astype(np.int16)) == 127)),)))

    def condition(tag, tiles):
        x = rng.integers(-100, 101, tiles * n.cond_tile() + 17).astype("<i2")
        plan = np.array([PLAN_ENTRY] * (-(-x.size // BLOCK)), dtype=cond_spec.PLAN_DTYPE)
        y, blanked, clipped = cond_spec.condition(as_bytes(x), np.int16, 1, BLOCK, plan, 0)
        call = reads(lambda c, r: c.condition(r, np.int16, 1, BLOCK, plan, 0), "blanked", "clipped")
        return ("condition" + tag, as_bytes(x), call, (y, (blanked, clipped)))

    def unpack(tag, bits, tiles):
        # one field of every byte, so that any number of bytes is whole frames: an output per input byte
        frame, first = 8 // bits, 1
        b = rng.integers(0, 256, tiles * n.unpack_tile() + 17).astype(np.uint8)
        table = unpack_spec.table(bits)
        y = unpack_spec.unpack(b, bits, table, 0, frame, first, 1)
        counts = unpack_spec.code_counts(b, bits, 0, frame, first, 1)
        assert not counts[1 << bits:].any()
        def call(c, r):
            out = c.unpack(r, bits, table, frame=frame, first=first)
            return out, tuple(int(v) for v in out.code_counts)
        return ("unpack%d%s" % (bits, tag), as_bytes(b), call, (y, tuple(int(v) for v in counts[:1 << bits])))

    def combine_blocks():
        n_out = 3 * n.combine_tile() + 18                                      # two blocks of I/Q frames
        x = rng.integers(-100, 101, 3 * n_out).astype(np.int8)
        B = n.ARRAY_BLOCK_UNIT
        h = rng.integers(-3000, 3001, (-(-(n_out // 2) // B), 3, 3, 2)).astype(np.int16)
        y, count = array_block_spec.combine_blocks(x, h, B, 6, 2, 3)
        return ("combine_blocks", x, reads(lambda c, r: c.combine_blocks(r, 2, 3, h, B, 6), "clipped"), (y, (count,)))

    def excise(tag, tiles):
        # a strong line under noise that saturates, as the "rails" cases of tests/excise_cases.py: with the line cut,
        # samples on a rail move beyond it
        m = excise_cases.tile_span(64, tiles)
        x = excise_cases.to_int8(80.0 * np.cos(2.0 * np.pi * 0.2031 * np.arange(m)) + excise_cases.noise(rng, m, 60.0))
        y, info = excise_spec.excise(x, 64, 8.0, 3, margins=True)
        assert info["margin_compare"] >= excise_spec.MARGIN and info["margin_round"] >= excise_spec.MARGIN, info
        def call(c, r):
            out, got = c.excise_record(r, 64, 8.0, 3)
            return out, (got["bins_cut"], got["segments_cut"], got["clipped"])
        return ("excise" + tag, x, call, (y, (info["bins_cut"], info["segments_cut"], info["clipped"])))

    def cancel(tag, tiles, starts, seed):
        tile = cancel_cases.TILE
        rows = [(prn, dop, cp, cancel_cases.CHIP_RATE + np.array([1.5, -2.5])) for prn, dop, cp in zip((9, 23), (1800.0, -3300.0),
                                                                                                     starts)]
        c = cancel_cases.handmade_case(seed, rows, 2, 250.0, length=tiles * tile + 17)
        assert bytes(n.settings_struct(c["s"])) == bytes(n.settings_struct(cancel_settings()))
        y, v, clipped, covered = cancel_spec.cancel(c["s"], c["x"], 0, c["chans"], c["series"], None, c["amp"])
        assert not cancel_spec.decisions(v, covered).any(), "cancel%s: a rounding decision - take another seed" % tag
        over = np.flatnonzero(covered & (np.abs(np.rint(v)) > 127.0)) // tile
        assert over.size == clipped and set(over.tolist()) >= set(s // tile for s in starts), (tag, set(over.tolist()))
        call = reads(lambda ctx, r: ctx.if_cancel(r, c["chans"], c["series"], c["amp"]), "clipped")
        return ("cancel" + tag, c["x"], call, (y, (clipped,)))

    cases += [requantize("", 3), condition("", 3), unpack("", 2, 3), unpack("", 4, 3), combine_blocks(), excise("", 3),
              requantize("_257", 257), condition("_257", 257), unpack("_257", 4, 257), excise("_257", 257),
              cancel("", 3, (7, 4096 + 2100), 31), cancel("_257", 257, (1, 256 * 4096 + 3), 32)]
    sizes = {"requantize": 3 * n.requant_tile() + 17, "condition": 3 * n.cond_tile() + 17, "unpack2": 3 * n.unpack_tile() + 17,
             "unpack4": 3 * n.unpack_tile() + 17, "combine_blocks": 3 * n.combine_tile() + 18,
             "requantize_257": 257 * n.requant_tile() + 17, "condition_257": 257 * n.cond_tile() + 17,
             "unpack4_257": 257 * n.unpack_tile() + 17, "cancel": 3 * cancel_cases.TILE + 17,
             "cancel_257": 257 * cancel_cases.TILE + 17}
    for name, x, _, (y, counts) in cases:
        assert y.size == sizes.get(name, y.size), (name, y.size)
        assert all(v == 0 for v in counts) if name == "resample" else all(v > 0 for v in counts), (name, counts)
    assert [len(counts) for _, _, _, (_, counts) in cases] == [1, 1, 1, 1, 2, 4, 16, 1, 3, 1, 2, 16, 3, 1, 1]
    return cases


def cancel_settings():
    """The settings of the context the walk runs on: the cancellation reads the sampling frequency, and at 2.046 Msps a block
    is half a tile.  No other stage of the walk reads a setting."""
    return orc.OracleSettings(samplingFreq=cancel_cases.LOW_FS, IF=cancel_cases.LOW_IF, numberOfChannels=2, msToProcess=2.0)


def every_ordered_pair(n):
    """A walk over 0 .. n - 1 on which every ordered pair (a, b), a == b included, occurs once as (a stop, the next stop):
    an Euler circuit of the complete directed graph with loops, n^2 + 1 stops (Hierholzer)."""
    left = [list(range(n)) for _ in range(n)]
    stack, walk = [0], []
    while stack:
        if left[stack[-1]]:
            stack.append(left[stack[-1]].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert sorted(zip(walk, walk[1:])) == [(a, b) for a in range(n) for b in range(n)]
    return walk


def test_the_fir_stages_share_one_clip_area_and_each_count_is_its_own():
    """Every stage that counts shares one counter area, so a call could read what the call before it left there.  On one
    context ALL ordered pairs (first, second) of the fifteen cases of counter_area_cases() run, a case behind itself
    included: the calls follow a walk on which every pair occurs once as neighbours, 226 calls, and every call's record
    equals its spec in bytes and every one of its counters the spec's - among them each stage with one counter behind the
    4-bit unpacker, which fills all 16 words of a slot, and behind the excision, which fills three.  The context has the
    cancellation's sampling frequency (cancel_settings)."""
    cases = counter_area_cases()
    ctx = pkg().engine.get_context(cancel_settings(), 0)
    for i in every_ordered_pair(len(cases)):
        name, x, call, (want, counts) = cases[i]
        rec = ctx.upload(x)
        try:
            out, got = call(ctx, rec)
        finally:
            rec.free()
        try:
            print(name, "counters", got, "spec", counts)
            assert tuple(got) == tuple(counts), (name, got, counts)
            assert out.download().tobytes() == want.tobytes(), name
        finally:
            out.free()
