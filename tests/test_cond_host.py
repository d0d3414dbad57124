"""CPU-only checks of the front-end conditioning stage (include/sgx.h: sgx_cond_plan, and the argument refusals of
sgx_cond_block_stats / sgx_if_condition that need no device) against the numpy contract of tests/cond_spec.py; the exports
and the struct layouts; the contract's overflow bounds; the Settings surface."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import cond_cases as cases
import cond_spec as spec
import requant_spec
from conftest import ROOT, pkg

NEW_SYMBOLS = ("sgx_cond_block_stats", "sgx_cond_plan", "sgx_cond_tile", "sgx_cond_timing", "sgx_if_condition")


@pytest.fixture(scope="module")
def built():
    importlib.import_module("__graft_entry__").build()
    return pkg()


def test_exports_and_layout(built):
    n = built._native
    raw = open(os.path.join(ROOT, "include", "sgx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sgx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(n.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in n.SYMBOLS and hasattr(lib, s), s
    for name, struct, dtype, want, size in (("sgx_cond_stats", n.CondStats, n.COND_STATS_DTYPE, spec.STATS_DTYPE, 64),
                                            ("sgx_cond_entry", n.CondEntry, n.COND_PLAN_DTYPE, spec.PLAN_DTYPE, 24)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S)
        fields = [f.strip() for decl in m.group(1).split(";") if decl.strip()
                  for f in decl.replace("int64_t", "").replace("int32_t", "").split(",")]
        assert fields == [f[0] for f in struct._fields_] == list(want.names) == list(dtype.names), name
        assert C.sizeof(struct) == size == want.itemsize == dtype.itemsize
        assert [getattr(struct, f).offset for f in fields] == [want.fields[f][1] for f in fields] == \
            [dtype.fields[f][1] for f in fields]
    assert n.COND_OFFSET_BINARY == 1 and "#define SGX_COND_OFFSET_BINARY 1" in raw
    assert n.cond_type("int8") == (0, 1, 0) and n.cond_type("uint8") == (0, 1, 1) and n.cond_type("<i2") == (1, 2, 0)
    assert n.cond_tile() > 0 and n.cond_tile() % 16 == 0
    assert "tests/cond_spec.py" in raw


# ---- the plan ----------------------------------------------------------------------------------------------------------------

def stats_rows(rows):
    """STATS_DTYPE from (n, kept, dc0, dc1, p_kept) rows."""
    st = np.zeros(len(rows), dtype=spec.STATS_DTYPE)
    for i, (nk, kept, dc0, dc1, p) in enumerate(rows):
        st[i] = (nk, kept, dc0, dc1, p, p, 0, 0)
    return st


def hand_made():
    """(name, statistics, lanes): a level step of 18 dB, a block with p_kept = 0, K = 1, DC of +-2^19, powers over 40
    decades, kept = 1 and kept = n."""
    rng = np.random.default_rng(11)
    p0 = 416 * 2 * 256 * 96 ** 2
    step = [(416, 400 + i % 7, 1150 + i, -700 - i, p0 + 1000 * i) for i in range(40)]
    step += [(416, 410 - i % 5, 9200 - i, -5600 + i, 64 * p0 - 777 * i) for i in range(40)]
    zero = step[:5] + [(416, 416, 3, -3, 0)] + step[5:10]
    dcs = [(256, 256, (1 << 19), -(1 << 19), 10 ** 9), (256, 256, -(1 << 19), (1 << 19), 10 ** 9 + 1),
           (256, 200, (1 << 19) - 1, 1 - (1 << 19), 3)] * 4
    wide = [(16384, int(rng.integers(1, 16385)), int(rng.integers(-1000, 1000)), int(rng.integers(-1000, 1000)), 0)
            for _ in range(200)]
    wide = [(a, k, d0, d1, int(k * float(np.exp(rng.uniform(0.0, 29.0))))) for a, k, d0, d1, _ in wide]
    return [("step", stats_rows(step), 2), ("step1", stats_rows(step), 1), ("zero", stats_rows(zero), 2),
            ("all zero", stats_rows([(256, 256, 0, 0, 0)] * 3), 1), ("one", stats_rows(step[:1]), 2),
            ("none", stats_rows([]), 2), ("dc", stats_rows(dcs), 2), ("wide", stats_rows(wide), 2),
            ("kept one", stats_rows([(300, 1, 5, 6, (1 << 43) - 1), (300, 1, 5, 6, 0), (300, 300, 5, 6, 300 << 42)]), 2)]


def scene_stats():
    x = cases.capture()[:40 * cases.SCENE.samples_per_code]
    out = [("scene", spec.block_stats(x, x.dtype, 2, cases.BLOCK, cases.BLANK_Q4), 2),
           ("scene as real", spec.block_stats(x, x.dtype, 1, 256, 16), 1)]
    y = np.random.default_rng(12).integers(-128, 128, 70000).astype(np.int8)
    out.append(("int8", spec.block_stats(y, "int8", 2, 272, 4096), 2))
    out.append(("uint8", spec.block_stats(y.view(np.uint8), "uint8", 1, 16384, 0), 1))
    return out


def test_plan_equals_the_contract(built):
    n = built._native
    seen = 0
    for name, st, lanes in hand_made() + scene_stats():
        for q4 in (0, 16, 256, 4096):
            for target in (12.0, 127.0, 0.37):
                for agc in (1.0, 32.0, 1000.0, 2.5):
                    want = spec.plan(st, lanes, q4, target, agc)
                    got = n.cond_plan(st, lanes, q4, target, agc)
                    assert got.dtype == spec.PLAN_DTYPE and got.tobytes() == want.tobytes(), (name, q4, target, agc)
                    spec.check_plan(want, st.size)
                    seen += want.size
    assert seen > 10000
    # by hand.  One block at rms 96 LSB per lane: a = 96^2, g = 12 / 96 = 2^-3 -> (16384, 17); theta = 96^2 * 16 * 2 * 256
    st = stats_rows([(416, 416, 1152, -704, 416 * 2 * 256 * 96 ** 2)])
    p = spec.plan(st, 2, 256, 12.0, 32.0)
    assert p.tolist() == [(1152, -704, 16384, 17, 96 ** 2 * 16 * 2 * 256)]
    assert requant_spec.gain(1, 96.0 ** 2, 12.0)[:2] == (16384, 17) == spec.mult_shift(0.125)
    # alpha = 1: every block stands for itself; blank_q4 = 0: INT64_MAX; p_kept = 0: the gain is 1, theta 0
    step = hand_made()[0][1]
    p = spec.plan(step, 2, 0, 12.0, 1.0)
    assert np.array_equal(p["dc0"], step["dc0"]) and np.all(p["theta"] == spec.INT64_MAX)
    assert p["shift"][-1] - p["shift"][0] == 3                       # 18 dB up: the gain falls by 2^3
    z = spec.plan(stats_rows([(256, 256, 0, 0, 0)]), 1, 256, 12.0, 1.0)
    assert z.tolist() == [(0, 0, 16384, 14, 0)]
    # alpha = 1 / 1000 hardly moves: 40 blocks at 64 x the power raise a by 1 + 63 (1 - 0.999^40) = 3.47, the gain falls
    # by 5.4 dB of the 18
    slow = spec.plan(step, 2, 256, 12.0, 1000.0)
    g = slow["mult"] / np.exp2(slow["shift"].astype(float))
    assert abs(20 * np.log10(g[39] / g[0])) < 0.05
    assert abs(20 * np.log10(g[-1] / g[0]) + 10 * np.log10(1 + 63 * (1 - 0.999 ** 40))) < 0.2
    # half-even rounding of the DC: A = 2.5 -> 2, 3.5 -> 4, -2.5 -> -2
    h = spec.plan(stats_rows([(256, 256, 2, 3, 1000), (256, 256, 3, 4, 1000), (256, 256, 0, -6, 1000)]), 2, 16, 12.0, 2.0)
    assert h["dc0"].tolist() == [2, 2, 1] and h["dc1"].tolist() == [3, 4, -1]


def test_refusals_before_the_device(built):
    """B = 255, B = 16400, B no multiple of 16, L = 3, odd n with L = 2, offset binary with int16, G = 65, blank_q4 = 15:
    SGX_E_ARG in the library, ValueError in the contract."""
    n = built._native
    f = n.lib()
    out = C.c_void_p()
    k = C.c_size_t(0)
    st = (n.CondStats * 4)()
    plan = (n.CondEntry * 4)()

    def stats_rc(dt=n.DT_INT16, lanes=2, block=256, q4=256, flags=0):
        return f.sgx_cond_block_stats(None, None, dt, lanes, block, q4, flags, st, 4, C.byref(k))

    def apply_rc(dt=n.DT_INT16, lanes=2, block=256, flags=0, guard=8):
        return f.sgx_if_condition(None, None, dt, lanes, block, flags, plan, 4, guard, C.byref(out), None, None)

    # good arguments get as far as the missing context
    assert stats_rc() == n.SGX_E_ARG and "c && rec" in n.last_error()
    assert apply_rc() == n.SGX_E_ARG and "c && rec" in n.last_error()
    assert stats_rc(n.DT_INT8, 1, 16384, 0, 1) == n.SGX_E_ARG and "c && rec" in n.last_error()
    assert apply_rc(n.DT_INT8, 1, 16384, 1, 64) == n.SGX_E_ARG and "c && rec" in n.last_error()
    for block in (255, 16400, 264, 0, -256, 16385):
        assert stats_rc(block=block) == n.SGX_E_ARG and "block" in n.last_error(), block
        assert apply_rc(block=block) == n.SGX_E_ARG and "block" in n.last_error(), block
        with pytest.raises(ValueError):
            spec.check_record(1024, "int16", 2, block)
    for lanes in (3, 0, -1):
        assert stats_rc(lanes=lanes) == n.SGX_E_ARG and "lanes" in n.last_error()
        assert apply_rc(lanes=lanes) == n.SGX_E_ARG and "lanes" in n.last_error()
        with pytest.raises(ValueError):
            spec.check_record(1024, "int16", lanes, 256)
        with pytest.raises(ValueError):
            spec.check_plan_args(lanes, 256, 12.0, 32.0)
        assert f.sgx_cond_plan(st, 0, lanes, 256, 12.0, 32.0, plan) == n.SGX_E_ARG and "lanes" in n.last_error()
    assert stats_rc(flags=n.COND_OFFSET_BINARY) == n.SGX_E_ARG and "OFFSET_BINARY" in n.last_error()
    assert apply_rc(flags=n.COND_OFFSET_BINARY) == n.SGX_E_ARG and "OFFSET_BINARY" in n.last_error()
    assert stats_rc(dt=n.DT_INT8, flags=2) == n.SGX_E_ARG and "flags" in n.last_error()
    with pytest.raises(ValueError):
        spec.width("int16", offset_binary=True)
    for dt in (n.DT_UINT8, n.DT_FLOAT32, n.DT_FLOAT64, -1, 11):
        assert stats_rc(dt=dt) == n.SGX_E_ARG and "data_type" in n.last_error()
        assert apply_rc(dt=dt) == n.SGX_E_ARG and "data_type" in n.last_error()
    for name in ("float32", "uint16", "float64"):
        with pytest.raises(ValueError):
            spec.width(name)
        with pytest.raises(ValueError):
            n.cond_type(name)
    for guard in (65, -1, 1000):
        assert apply_rc(guard=guard) == n.SGX_E_ARG and "guard" in n.last_error()
        with pytest.raises(ValueError):
            spec.check_guard(guard)
    spec.check_guard(0), spec.check_guard(64)
    for q4 in (15, 1, -16, 4097):
        assert stats_rc(q4=q4) == n.SGX_E_ARG and "blank_q4" in n.last_error()
        assert f.sgx_cond_plan(st, 0, 2, q4, 12.0, 32.0, plan) == n.SGX_E_ARG and "blank_q4" in n.last_error()
        with pytest.raises(ValueError):
            spec.check_record(1024, "int16", 2, 256, q4)
        with pytest.raises(ValueError):
            spec.check_plan_args(2, q4, 12.0, 32.0)
    # odd n with L = 2, bytes that split an element: the contract's side (the library looks at the record:
    # tests/test_cond_gpu.py)
    for nbytes, dt, lanes in ((1001, "int8", 2), (1002, "int16", 2), (1001, "int16", 1)):
        with pytest.raises(ValueError):
            spec.check_record(nbytes, dt, lanes, 256)
        with pytest.raises(ValueError):
            spec.frames(np.zeros(nbytes, dtype=np.uint8), dt, lanes)
    # the plan's own arguments
    for target in (0.0, -1.0, 127.0000001, float("nan"), float("inf")):
        assert f.sgx_cond_plan(st, 0, 2, 256, target, 32.0, plan) == n.SGX_E_ARG and "target_rms" in n.last_error()
        with pytest.raises(ValueError):
            spec.check_plan_args(2, 256, target, 32.0)
    for agc in (0.0, 0.999, -5.0, float("nan"), float("inf")):
        assert f.sgx_cond_plan(st, 0, 2, 256, 12.0, agc, plan) == n.SGX_E_ARG and "agc_blocks" in n.last_error()
        with pytest.raises(ValueError):
            spec.check_plan_args(2, 256, 12.0, agc)
    assert f.sgx_cond_plan(None, 1, 2, 256, 12.0, 32.0, plan) == n.SGX_E_ARG
    assert f.sgx_cond_plan(st, 1, 2, 256, 12.0, 32.0, plan) == n.SGX_E_ARG and "kept" in n.last_error()   # kept = 0
    with pytest.raises(ValueError):
        spec.plan(np.zeros(1, dtype=spec.STATS_DTYPE), 2, 256, 12.0, 32.0)
    assert f.sgx_cond_plan(None, 0, 2, 256, 12.0, 32.0, None) == n.SGX_OK
    assert f.sgx_cond_timing(None, None, None) == n.SGX_E_ARG and "stats_ms" in n.last_error()
    assert f.sgx_cond_tile(None) == n.SGX_E_ARG and "tile_frames" in n.last_error()
    # plan entries out of range: the contract's side
    good = np.zeros(2, dtype=spec.PLAN_DTYPE)
    good["mult"] = 1
    spec.check_plan(good, 2)
    for field, v in (("mult", 0), ("mult", 32768), ("shift", 31), ("shift", -1), ("dc0", (1 << 20) + 1),
                     ("dc1", -(1 << 20) - 1), ("theta", -1)):
        bad = good.copy()
        bad[field][1] = v
        with pytest.raises(ValueError):
            spec.check_plan(bad, 2)
    with pytest.raises(ValueError):
        spec.check_plan(good, 3)


def test_overflow_bounds_of_the_contract():
    """A block of 16384 frames of (-32768, 32767) pairs, and the same with the rails alternating: every intermediate stays
    inside the bounds the header states, and inside int64."""
    B = 16384
    x = np.empty((B, 2), dtype="<i2")
    x[:, 0], x[:, 1] = -32768, 32767
    alt = x.copy()
    alt[1::2, 0], alt[1::2, 1] = 32767, -32768
    for rec, d_max in ((x, 0), (alt, 16 * 32768)):
        st = spec.block_stats(rec, "int16", 2, B, 4096)
        assert st.size == 1 and st["n"][0] == st["kept"][0] == B
        d = 16 * rec.astype(np.int64) - np.array([st["dc0"][0], st["dc1"][0]])
        assert np.abs(d).max() < 1 << 21 and abs(int(np.abs(d).max()) - d_max) <= 16
        e = (d * d).sum(axis=1)
        assert int(e.max()) < 1 << 43 and int(e.max()) == st["e_max"][0]
        assert int(e.sum()) < 1 << 57 and int(e.sum()) == st["p_all"][0] == st["p_kept"][0]
        assert (int(st["p_all"][0]) // B) * 4096 < 1 << 63                        # theta_r before its shift
    assert abs(int(st["dc0"][0])) <= 8 and st["p_all"][0] > 1 << 52                # the alternating block: all power, no DC
    st = spec.block_stats(x, "int16", 2, B, 4096)
    assert (st["dc0"][0], st["dc1"][0], st["p_all"][0]) == (-(1 << 19), (1 << 19) - 16, 0)
    # the worst plan and the worst product of the quantiser: |d| < 2^21, mult < 2^15, the rounding term 2^33
    p = spec.plan(spec.block_stats(alt, "int16", 2, B, 4096), 2, 4096, 127.0, 1.0)
    assert 0 <= p["theta"][0] < 1 << 62
    assert ((1 << 21) * 32767 + (1 << 33)) < 1 << 63
    worst = np.zeros(1, dtype=spec.PLAN_DTYPE)
    worst[0] = (-(1 << 20), 1 << 20, 32767, 0, spec.INT64_MAX)
    y, blanked, clipped = spec.condition(alt, "int16", 2, B, worst, 64)
    assert blanked == 0 and clipped == 2 * B and set(np.unique(y)) == {-127, 127}
    # one lane, int8, offset binary: the same bounds hold a fortiori
    u = np.zeros(B, dtype=np.uint8)
    u[1::2] = 255
    st = spec.block_stats(u, "uint8", 1, B, 16)
    assert (st["dc0"][0], st["p_all"][0]) == (-8, B * (16 * 128 - 8) ** 2)


# ---- Settings --------------------------------------------------------------------------------------------------------------------

def test_settings_surface(built):
    s = built.Settings()
    assert (s.frontEndConditioning, s.condBlockUs, s.condAgcBlocks, s.condBlankFactor, s.condGuardFrames, s.condTargetRms) == \
        (False, cases.BLOCK_US, cases.AGC_BLOCKS, cases.BLANK_FACTOR, cases.GUARD, cases.TARGET_RMS)
    assert s._prepared_settings() is s                                     # off: nothing changes
    with pytest.raises(ValueError, match="frontEndConditioning"):
        s.conditionRecord(None)
    s.frontEndConditioning = True
    # the block: 100 us at 38.192 MHz = 3819.2 frames -> 3824; clamped at both ends
    assert s._cond_format() == (1, 1, 3824, 256) and spec.block_frames(s.samplingFreq, s.condBlockUs) == 3824
    s.condBlockUs = 1.0
    assert s._cond_format()[2] == 256
    s.condBlockUs = 1e6
    assert s._cond_format()[2] == 16384
    s.condBlockUs, s.condBlankFactor = 100.0, 0.0
    assert s._cond_format()[3] == 0
    s.condBlankFactor = 4.0
    # a real int16 record is read as int8 afterwards, its skip as a sample
    s.dataType, s.skipNumberOfBytes = 'int16', 4000
    real = s._prepared_settings()
    assert (real.dataType, real.skipNumberOfBytes, real.frontEndConditioning, real.samplingFreq) == ('int8', 2000, False,
                                                                                                     s.samplingFreq)
    assert s.dataType == 'int16' and s.skipNumberOfBytes == 4000 and s._cond_format()[:2] == (2, 1)
    assert built._native.track_plan(real, built._native.DT_INT8, 8)[0] == 5          # trk3_kernel
    s.skipNumberOfBytes = 4001
    with pytest.raises(ValueError, match="skipNumberOfBytes = 4001"):
        s._prepared_settings()
    s.skipNumberOfBytes = 0
    s.dataType = 'uint8'
    assert s._prepared_settings().dataType == 'int8' and s._cond_format()[0] == 1
    # I/Q: two lanes; the converter sees int8 without an offset whatever the file held
    s.iqRecord, s.samplingFreq, s.IF = True, 4096000.0, 0.0
    for dt, w in (('int8', 1), ('uint8', 1), ('int16', 2)):
        s.dataType = dt
        assert s._cond_format() == (w, 2, 416, 256) and s._iq_format() == (False, False) and s._iq_width() == w
        real = s._prepared_settings()
        assert (real.dataType, real.iqRecord, real.frontEndConditioning, real.samplingFreq) == ('int8', False, False, 8192000.0)
    s.skipNumberOfBytes = 6
    with pytest.raises(ValueError, match="skipNumberOfBytes = 6"):
        s.postProcessing("/nonexistent/record.bin")
    s.skipNumberOfBytes = 0
    # the refused combinations
    s.dataType = 'float32'
    with pytest.raises(ValueError, match="float32"):
        s.postProcessing("/nonexistent/record.bin")
    s.dataType, s.iqRequantize = 'int16', True
    with pytest.raises(ValueError, match="iqRequantize"):
        s.postProcessing("/nonexistent/record.bin")
    s.iqRequantize, s.iqRecord = False, False
    s.dataType = 'float32'
    with pytest.raises(ValueError, match="float32"):
        s.postProcessing("/nonexistent/record.bin")
    s.dataType = 'uint16'
    with pytest.raises(ValueError, match="int8, uint8 and int16"):
        s.postProcessing("/nonexistent/record.bin")
