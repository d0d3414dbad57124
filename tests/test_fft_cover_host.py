"""The radix-pass case table (tests/fft_cover.py) without a GPU: that its lengths put every radix of csrc/sgx_fft.hip into
every position a pass can take - asserted from what sgx_acquire_fft_passes reports, not from a list written by hand - that
it holds last passes of more than 64 workgroups and both kinds of last workgroup, and that every acquisition scene
tests/test_fft_gpu.py asserts exactly is well conditioned in numpy alone (the rules of tests/test_any_rate_host.py: no
asserted arg-max within 1e-6 of its runner-up, no peakMetric within 1 % of the threshold) and puts a detection into every
slot of the last radix."""
import numpy as np
import pytest

import any_rate
import fft_cover as fc
from conftest import pkg
from oracle import softgnss_oracle as orc


def test_plan_export_agrees_with_the_length_export_and_multiplies_out():
    nat = pkg()._native
    for n in fc.LENGTHS + any_rate.SMOOTH_IN_USE + [53000, 37000, 5714]:
        c = fc.Case(n)
        assert c.length == nat.acquire_fft_length(n)
        assert int(np.prod(c.radices, dtype=np.int64)) == c.length, n
        assert set(c.radices) <= set(fc.RADICES) and len(c.tpb) == len(c.radices)
        assert all(t in (64, 128, 256) for t in c.tpb)
        assert c.blocks == -(-c.ns_last // c.tpb_last)
        assert c.padded == (not any_rate.smooth(n)) and (not c.padded or c.length >= 2 * n - 1)
    # one radix, one width, whatever the position
    width = {}
    for n in fc.LENGTHS:
        c = fc.plan(n)
        for r, t in zip(c.radices, c.tpb):
            assert width.setdefault(r, t) == t
    assert sorted(width) == sorted(fc.RADICES)


def test_plan_export_refuses_what_the_length_export_refuses():
    nat = pkg()._native
    for n in (0, 1, -5, 2 ** 29 + 1):
        with pytest.raises(nat.SgxError):
            nat.acquire_fft_passes(n)


def test_every_radix_runs_in_every_position():
    cov = fc.coverage()
    want = set(fc.RADICES)
    assert len(fc.LENGTHS) == len(set(fc.LENGTHS))
    assert all(not fc.plan(n).padded for n in fc.FACTORING) and all(fc.plan(n).padded for n in fc.PADDED)
    assert all(2000 <= n <= 131072 and len(fc.plan(n).radices) >= 2 for n in fc.LENGTHS)
    for pos in ("first", "middle", "last", "last_padded"):
        assert cov[pos] == want, (pos, sorted(want - cov[pos]))


def test_table_holds_many_workgroups_and_both_kinds_of_last_workgroup():
    many = [n for n in fc.LENGTHS if fc.plan(n).blocks > fc.MANY_BLOCKS]
    assert {100000, 98304, 131072} <= {n for n in many if not fc.plan(n).padded}
    assert len([n for n in many if fc.plan(n).padded]) >= 2
    for padded in (False, True):
        kinds = {fc.plan(n).partial for n in fc.LENGTHS if fc.plan(n).padded == padded}
        assert kinds == {False, True}, padded
    assert not fc.plan(fc.NONCOH_N).padded and fc.plan(fc.NONCOH_N).blocks > fc.MANY_BLOCKS
    assert not fc.plan(fc.DEFERRED_N).padded and fc.plan(fc.DEFERRED_N).blocks > fc.MANY_BLOCKS


@pytest.mark.parametrize("n", fc.LENGTHS)
def test_fused_inputs_name_every_slot_and_edge(n):
    c = fc.plan(n)
    idx = dict(fc.dominant_indices(c))
    assert {idx["slot%d" % q] // c.ns_last for q in range(c.last)} == set(range(c.last))
    assert all(0 <= i < c.length for i in idx.values())
    lane = lambda i: (i % c.ns_last) % c.tpb_last
    wg = lambda i: (i % c.ns_last) // c.tpb_last
    assert lane(idx["first_wg_lane0"]) == 0 and wg(idx["first_wg_lane0"]) == 0
    assert wg(idx["first_wg_last_lane"]) == 0 and lane(idx["first_wg_last_lane"]) == min(c.tpb_last, c.ns_last) - 1
    assert wg(idx["last_wg_lane0"]) == c.blocks - 1 and lane(idx["last_wg_lane0"]) == 0
    assert wg(idx["last_wg_last_live_lane"]) == c.blocks - 1
    assert (lane(idx["last_wg_last_live_lane"]) != c.tpb_last - 1) == c.partial


@pytest.mark.parametrize("n", fc.LENGTHS)
def test_acquisition_scenes_are_well_conditioned_and_fill_every_slot(n):
    c = fc.plan(n)
    won = set()
    for prns, phases, x in fc.scene_records(n):
        o = fc.oracle_settings(n, prns)
        assert o.samplesPerCode == n
        w, gap, room = any_rate.conditioned(o, x, 2, False, prns)
        ref = orc.acquire(o, x)
        print("\n%d: smallest gap %.2e, closest metric to the threshold %.3f" % (n, gap, room))
        for k in ("carrFreq", "codePhase", "freqBin", "fineIdx"):
            assert np.array_equal(w[k], ref[k]), k
        assert gap >= fc.GAP, gap
        assert room >= fc.THRESHOLD_ROOM, room
        assert all(ref["carrFreq"][p - 1] > 0 for p in prns), ref["peakMetric"][:len(prns)]
        # (the peak lies within a sample of where the scene puts the code's start, and in that slot)
        for p, want in zip(prns, phases):
            got = int(ref["codePhase"][p - 1])
            assert abs(got - want) <= 1 and got // c.ns_last == want // c.ns_last, (p, got, want)
        won |= fc.winning_slots(c, ref, prns)
    assert won == set(c.slots()) and (c.padded or len(won) == c.last)


def test_noncoherent_scene_is_well_conditioned():
    n = fc.NONCOH_N
    prns, phases, x = fc.scene_records(n)[0]
    o = fc.oracle_settings(n, prns)
    w, gap, room = any_rate.conditioned(o, x, 4, True, prns)
    ref = orc.acquire(o, x, n_blocks=4, noncoh=True)
    for k in ("carrFreq", "codePhase", "freqBin", "fineIdx"):
        assert np.array_equal(w[k], ref[k]), k
    assert gap >= fc.GAP and room >= fc.THRESHOLD_ROOM, (gap, room)
    assert all(ref["carrFreq"][p - 1] > 0 for p in prns)
