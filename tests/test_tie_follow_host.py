"""The tie follower (tests/tie_follow.py) is the judge of the full-length GPU runs, so it is tested by mutation here, on
the CPU: a 60 ms stretch of the host-generated default scene, `got` made from the oracle's own stepper with known flips
or known damage, and the verdict the follower must reach for each.

Every block of this front end has a sample within 4.5e-3 chips of a chip boundary (the samples sit on a near-periodic
raster of 112 per 3 chips), so D = 1e-2 makes ties available everywhere and D = 1e-11 / D = 0 nowhere: the same `got`
must be `ties` under the first and `defect` under the others."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import softgnss_oracle as orc
import tie_follow as tf

MS = 60
WIDE = 1e-2          # a D under which every block offers ties (see above)


@pytest.fixture(scope="module")
def base(default_record):
    """(record, [channel 0, channel 1] of the tracking golden, oracle settings, their plain runs)."""
    g = load_golden("trk_default.npz")
    rec = default_record[:(MS + 10) * 38192]
    chans = [(int(g["ch_PRN"][i]), float(g["ch_acquiredFreq"][i]), float(g["ch_codePhase"][i])) for i in range(2)]
    so = orc.OracleSettings(numberOfChannels=1, msToProcess=float(MS))
    return rec, chans, so, [tf.plain_run(rec, c, so, MS) for c in chans]


def _run(rec, chan, so, flips, ms=MS):
    """The stepper's series with flips = {block: [(arm, n), ...]}, everything else in the oracle's arithmetic."""
    st = tf.stepper(rec, chan, so)
    return np.array([st.step(flips.get(k, ())) for k in range(ms)]).T


def _at(rec, chan, so, plain, k):
    st = tf.stepper(rec, chan, so)
    st.restore(plain[1][0])
    for _ in range(k):
        st.step()
    return st


def _chips_differ(st, arm, n):
    t = st.ramps()[2][arm][n]
    c = int(np.ceil(t))
    return st.code[c] != st.code[c + (orc.flip_direction(t) if t != np.round(t) else 1)]


def _nearest_flip(rec, chan, so, plain, first=5):
    """(block >= first, arm, n, distance): the sample nearest to a chip boundary in its block, in the first block where
    that sample's two neighbouring chips differ (so that the sums do change)."""
    for k in range(first, MS):
        st = _at(rec, chan, so, plain, k)
        arm, n, d = st.eligible(0.5)[0]
        if _chips_differ(st, arm, n):
            return k, arm, n, d
    raise AssertionError("no block with a usable nearest sample")


def test_stepper_reproduces_track_and_resumes_from_a_state(base):
    rec, chans, so, plains = base
    table = dict(PRN=np.array([c[0] for c in chans]), acquiredFreq=np.array([c[1] for c in chans]),
                 codePhase=np.array([c[2] for c in chans]), status=['T', 'T'])
    so2 = orc.OracleSettings(numberOfChannels=2, msToProcess=float(MS))
    want = orc.stack_series(orc.track(so2, table, rec))
    for c in range(2):
        assert np.array_equal(plains[c][0], want[c])
    st = _at(rec, chans[0], so, plains[0], 30)
    saved = st.state()
    a = [st.step() for _ in range(30)]
    st.restore(saved)
    assert [st.step() for _ in range(30)] == a
    assert np.array_equal(np.array(a).T, want[0][:, 30:])
    # a short read changes nothing and says so
    short = tf.stepper(rec[:int(chans[0][2]) + 1000], chans[0], so)
    s0 = short.state()
    assert short.step() is None and short.state() == s0


def test_moved_helpers_agree_with_the_stepper(base):
    """rem_at / nearest_boundary (what tools/r6_parity_rate.py used to carry) restate the stepper's state from a recorded
    series: the same code phase, rate and nearest sample."""
    rec, chans, so, plains = base
    for k in (0, 1, 17, 44):
        st = _at(rec, chans[0], so, plains[0], k)
        rem, cf = tf.rem_at(plains[0][0], k)
        assert (rem, cf) == (st.rem_code, st.code_freq)
        d, arm, n = tf.nearest_boundary(rem, cf)
        near = st.eligible(0.5)
        if d > 0:
            assert d == near[0][2] and (arm, n) in {e[:2] for e in near if e[2] == d}
        else:
            assert all(e[2] > 0 for e in near)


def test_the_oracles_own_output_is_identical(base):
    rec, chans, so, plains = base
    for c in range(2):
        for plain in (None, plains[c]):
            r = tf.follow(plains[c][0], rec, chans[c], so, D=WIDE, plain=plain)
            assert r["verdict"] == "identical" and r["ties"] == [] and r["blocks_checked"] == MS, tf.describe(r)
            assert r["unflipped"]["max_rel_err_IQ"] == 0.0 and r["absoluteSample_identical"]


def test_one_flip_is_a_tie_under_a_wide_d_and_a_defect_under_the_real_one(base):
    rec, chans, so, plains = base
    k, arm, n, d = _nearest_flip(rec, chans[0], so, plains[0])
    assert 1e-9 <= d <= 1e-2, d
    got = _run(rec, chans[0], so, {k: [(arm, n)]})
    assert not np.array_equal(got[3:9, k], plains[0][0][3:9, k])                    # (the sums did change)
    r = tf.follow(got, rec, chans[0], so, D=WIDE, plain=plains[0])
    assert r["verdict"] == "ties", tf.describe(r)
    assert [(t["block"], t["arm"], t["n"]) for t in r["ties"]] == [(k, arm, n)], tf.describe(r)
    t = r["ties"][0]
    assert t["distance_chips"] == d and t["sample_value"] == float(rec[int(plains[0][0][0, k - 1]) + n])
    assert 0 < t["step_in_sums"] <= 2 * abs(t["sample_value"]) + 1e-9
    assert r["blocks_checked"] == MS and r["absoluteSample_identical"]
    assert r["unflipped_after_first_tie"]["max_rel_err_IQ"] < tf.TIGHT               # (0: the same arithmetic)
    # ... and the same series is a defect at that block when no sample is near enough: D as the project states it, and 0
    for dist in (tf.D_CHIPS, 0.0):
        r = tf.follow(got, rec, chans[0], so, D=dist, plain=plains[0])
        assert r["verdict"] == "defect" and r["first_offending"]["block"] == k, tf.describe(r)
        assert r["first_offending"]["eligible"] == 0 and r["ties"] == []
    # without the plain run handed in, the follower makes its own
    r = tf.follow(got, rec, chans[0], so, D=WIDE)
    assert r["verdict"] == "ties" and len(r["ties"]) == 1


def test_a_flip_far_from_every_boundary_is_a_defect(base):
    rec, chans, so, plains = base
    k = 7
    st = _at(rec, chans[0], so, plains[0], k)
    tp = st.ramps()[2]["P"]
    far = [int(n) for n in np.nonzero(np.abs(tp - np.round(tp)) >= 0.1)[0] if _chips_differ(st, "P", int(n))]
    got = _run(rec, chans[0], so, {k: [("P", far[len(far) // 2])]})
    r = tf.follow(got, rec, chans[0], so, D=WIDE, plain=plains[0])
    assert r["verdict"] == "defect" and r["first_offending"]["block"] == k, tf.describe(r)
    assert r["first_offending"]["eligible"] > 0                                      # (offered, none explains it)


def test_a_scaled_sum_is_a_defect_even_where_ties_are_on_offer(base):
    rec, chans, so, plains = base
    k = 9
    got = plains[0][0].copy()
    got[3, k] *= 1 + 1e-6
    r = tf.follow(got, rec, chans[0], so, D=WIDE, plain=plains[0])
    assert r["verdict"] == "defect" and r["first_offending"]["block"] == k, tf.describe(r)
    assert r["first_offending"]["eligible"] > 0 and r["first_offending"]["absoluteSample_equal"]
    assert "no flip" in r["first_offending"]["why"]


def test_a_shifted_block_boundary_is_a_defect(base):
    rec, chans, so, plains = base
    k = 11
    got = plains[0][0].copy()
    got[0, k:] += 1
    r = tf.follow(got, rec, chans[0], so, D=WIDE, plain=plains[0])
    assert r["verdict"] == "defect" and r["first_offending"]["block"] == k, tf.describe(r)
    assert r["first_offending"]["absoluteSample_equal"] is False
    # ... and after an adopted tie just the same
    k0, arm, n, _ = _nearest_flip(rec, chans[0], so, plains[0])
    got = _run(rec, chans[0], so, {k0: [(arm, n)]})
    got[0, k0 + 3:] += 1
    r = tf.follow(got, rec, chans[0], so, D=WIDE, plain=plains[0])
    assert r["verdict"] == "defect" and r["first_offending"]["block"] == k0 + 3 and len(r["ties"]) == 1, tf.describe(r)


def test_a_third_tie_in_one_channel_is_a_defect(base):
    rec, chans, so, plains = base
    flips, first = {}, 5
    for _ in range(3):                                   # each chosen along the trajectory the earlier flips leave
        st = tf.stepper(rec, chans[0], so)
        for k in range(MS):
            if k >= first:
                arm, n, d = st.eligible(0.5)[0]
                if _chips_differ(st, arm, n):
                    flips[k] = [(arm, n)]
                    first = k + 4
                    break
            st.step(flips.get(k, ()))
    blocks = sorted(flips)
    assert len(blocks) == 3
    got = _run(rec, chans[0], so, flips)
    r = tf.follow(got, rec, chans[0], so, D=WIDE, max_ties=2, plain=plains[0])
    assert r["verdict"] == "defect" and r["first_offending"]["block"] == blocks[2], tf.describe(r)
    assert "max_ties" in r["first_offending"]["why"] and [t["block"] for t in r["ties"]] == blocks[:2]
    r = tf.follow(got, rec, chans[0], so, D=WIDE, max_ties=3, plain=plains[0])        # (it is the cap that bit)
    assert r["verdict"] == "ties" and [t["block"] for t in r["ties"]] == blocks, tf.describe(r)


def test_a_sample_exactly_on_a_boundary_is_not_eligible_and_its_mutation_is_a_defect(base, monkeypatch):
    rec, chans, so, plains = base
    st = tf.stepper(rec, chans[0], so)
    assert st.block == 0 and st.rem_code == 0.0
    tp = st.ramps()[2]["P"]
    exact = [int(n) for n in np.nonzero(tp == np.round(tp))[0] if n > 0 and _chips_differ(st, "P", int(n))]
    assert len(exact) > 100 and all(n % 112 == 0 for n in exact)                      # (one every 112 samples)
    offered = {(arm, n) for arm, n, _ in st.eligible(0.5)}
    assert not offered & {("P", n) for n in exact}
    with pytest.raises(ValueError):
        st.step([("P", exact[3])])
    # the mutant the stepper refuses to make: that sample's chip index one up
    real = orc.flip_direction
    monkeypatch.setattr(orc, "flip_direction", lambda t: 1 if t == np.round(t) else real(t))
    got = _run(rec, chans[0], so, {0: [("P", exact[3])]})
    monkeypatch.undo()
    assert not np.array_equal(got[3:9, 0], plains[0][0][3:9, 0])
    for dist in (tf.D_CHIPS, WIDE):
        r = tf.follow(got, rec, chans[0], so, D=dist, plain=plains[0])
        assert r["verdict"] == "defect" and r["first_offending"]["block"] == 0, tf.describe(r)


def test_a_scene_is_followed_channel_by_channel(base):
    rec, chans, so, plains = base
    k, arm, n, _ = _nearest_flip(rec, chans[1], so, plains[1])
    got = np.stack([plains[0][0], _run(rec, chans[1], so, {k: [(arm, n)]})])
    assert not tf.diverges(got[0], plains[0]) and tf.diverges(got[1], plains[1])
    reports = tf.follow_scene(got, rec, chans, so, plains, D=WIDE)
    assert [r["verdict"] for r in reports] == ["identical", "ties"], "\n".join(tf.describe(r) for r in reports)
    assert [(t["block"], t["arm"], t["n"]) for t in reports[1]["ties"]] == [(k, arm, n)]
    cells = tf.eligible_blocks(rec, chans[1], so, MS, WIDE)
    assert (k, arm, n) in {c[:3] for c in cells} and tf.eligible_blocks(rec, chans[1], so, 20, 0.0) == []

