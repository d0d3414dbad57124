"""The excision stage's table (tests/excise_cases.py) conditioned in numpy alone: every case keeps every decision of the
contract (tests/excise_spec.py) at least spec.MARGIN from a rounding error, none left out, and the table covers what it
says it covers.  The library is loaded only for the tile size (sgx_excise_plan; needs no GPU).  Run with -m "not gpu"."""
import importlib

import numpy as np
import pytest

import excise_cases as cases
import excise_spec as spec


@pytest.fixture(scope="module", autouse=True)
def built():
    importlib.import_module("__graft_entry__").build()


def test_the_margin_is_a_hundred_times_the_transform_s_error():
    cmp_rel, o_abs = spec.fft_error_bound(spec.MAX_SEGMENT)
    assert 100.0 * cmp_rel <= spec.MARGIN and 100.0 * o_abs <= spec.MARGIN, (cmp_rel, o_abs)


def test_the_window_is_power_complementary():
    for N in (64, 256, 1024):
        w = spec.window(N)
        # two sines, two squares, a sum: a few roundings of 2^-53
        assert np.abs(w[:N // 2] ** 2 + w[N // 2:] ** 2 - 1.0).max() <= 8 * 2.0 ** -53


@pytest.mark.parametrize("c", cases.CASES, ids=[c.name for c in cases.CASES])
def test_every_case_is_well_conditioned(c):
    y, info = c.reference()
    print("%s: n %d, margins %.3g (compare) %.3g (round), cut %d bins in %d of %d segments, clipped %d"
          % (c.name, c.x.size, info["margin_compare"], info["margin_round"], info["bins_cut"], info["segments_cut"],
             info["segments"], info["clipped"]))
    assert info["margin_compare"] >= spec.MARGIN
    assert info["margin_round"] >= spec.MARGIN        # (a tie at a clip rail, +-127.5, is a half-integer too)
    assert y.size == c.x.size and info["segments"] == spec.segments(c.x.size, c.N)
    if "cut" in c.expect or "tile_cuts" in c.expect:
        assert info["bins_cut"] > 0
    if "clipped" in c.expect:
        assert info["clipped"] > 0 and (y == 127).any() and (y == -127).any()
    if "identity" in c.expect:
        assert info["bins_cut"] == 0 and np.array_equal(y, c.x)
    if "tile_cuts" in c.expect:
        S, per = cases.tile_segments(c.N), info["cut_per_segment"]
        assert info["segments"] > 3 * (S - 1)
        for t in (1, 2, 3):          # the segment two tiles share and its neighbours, the last and first of their own
            assert per[t * (S - 1) - 1] > 0 and per[t * (S - 1)] > 0 and per[t * (S - 1) + 1] > 0, t


def test_the_table_covers_what_it_says():
    by_n = {}
    for c in cases.CASES:
        by_n.setdefault(c.N, set()).add(c.x.size)
    for N in (64, 256, 1024):
        H = N // 2
        assert {1, H - 1, H, H + 1, N} <= by_n[N]
        assert any(n % H for n in by_n[N] if n > N)
    assert {c.passes for c in cases.CASES} >= {1, 3, 8}
    assert {c.threshold for c in cases.CASES} >= {1.0, 8.0}
    assert all(2000 <= c.x.size <= 400000 or c.name.startswith("len_") or c.x.size >= 4 * c.N for c in cases.CASES)


def test_a_clean_record_passes_nearly_unchanged():
    """Only the e^-threshold share of the noise bins goes."""
    c = cases.BY_NAME["noise_N256"]
    y, info = c.reference()
    share = info["bins_cut"] / float(info["segments"] * (c.N // 2 - 1))
    assert share < 4.0 * np.exp(-c.threshold)
