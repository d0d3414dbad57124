"""The full-scale records of tests/test_full_scale_gpu.py, checked in numpy: each int8 record the GPU tests call "below"
or "above" the speculative kernel's bound (sgx_trk3.hip: 2 048 bytes adding up to 131 072 in magnitude) is so, by a
stated margin - the GPU tests' expectations rest on these facts, not on assumed data.  No GPU needed."""
import numpy as np

from conftest import pkg
import full_scale as fsr

MS = 50


def test_int8_records_lie_on_the_stated_side_of_the_trk3_bound():
    m = pkg()
    s = m.Settings()
    recs = fsr.int8_records(m, s, MS)
    assert len(recs) == len(fsr.INT8_BELOW) + len(fsr.INT8_ABOVE) + 2
    for name, (x, above) in recs.items():
        assert x.dtype == np.int8, name
        kernel_w = fsr.window_mag_max(x, fsr.TRK3_WINDOW)
        host_w = fsr.window_mag_max(x, fsr.HOST_WINDOW)
        assert kernel_w <= host_w
        if above:
            # the kernel's own 2 048-byte window (the record wave's guard) reaches the bound: so does the host's wider one
            assert kernel_w >= (1 + fsr.MARGIN) * fsr.TRK3_BOUND, (name, kernel_w)
        else:
            # below even on the host scan's 2 176 bytes: no guard may send it away for its magnitudes
            assert host_w <= (1 - fsr.MARGIN) * fsr.TRK3_BOUND, (name, host_w)


def test_window_sum_matches_a_direct_sum():
    rng = np.random.default_rng(7)
    x = rng.integers(-128, 128, size=9000).astype(np.int8)
    want = max(int(np.abs(x[i:i + 2048].astype(np.int64)).sum()) for i in range(0, 9000 - 2048 + 1))
    assert fsr.window_mag_max(x, 2048) == want
    # int8 -128 has magnitude 128 (the kernels' v_sad_u8 of b ^ 0x80 against 0x80)
    assert fsr.window_mag_max(np.full(4096, -128, np.int8), 2048) == 128 * 2048


def test_clipped_and_saturated_records_sit_at_the_rails():
    m = pkg()
    s = m.Settings()
    for dtype, (lo, hi) in fsr.LIMITS.items():
        c = fsr.clipped_record(m, s, dtype, 5)
        assert c.dtype == np.dtype(dtype) and set(np.unique(c).tolist()) == {lo, hi}, dtype
        # the 1-bit record is the sign of the clean one
        x = fsr.clean_record(m, s, 1000, 5)
        assert np.array_equal(c == hi, x >= 0)
        sat = fsr.saturated_record(m, s, dtype, 5)
        assert sat.dtype == np.dtype(dtype)
        assert np.mean((sat == lo) | (sat == hi)) > 0.6, dtype     # clipping on most samples
    # the saturated int8 record is above the bound too (it is one of int8_records' "above" ones)
    assert fsr.window_mag_max(fsr.saturated_record(m, s, "int8", 5), 2048) >= (1 + fsr.MARGIN) * fsr.TRK3_BOUND


def test_float_records_are_the_integer_records_scaled_exactly():
    m = pkg()
    s = m.Settings()
    x = fsr.clean_record(m, s, 127, 3)
    for dt in (np.float32, np.float64):
        f = fsr.float_record(x, dt)
        assert f.dtype == dt and np.array_equal(f.astype(np.float64) / 2.0 ** 20, x.astype(np.float64))
    u = fsr.float_record(fsr.unrounded_record(m, s, 127, 3), np.float32)
    assert np.any(u / np.float32(2.0 ** 20) != np.rint(u / np.float32(2.0 ** 20)))      # not integers times 2^20
