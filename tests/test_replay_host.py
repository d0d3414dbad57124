"""Multi-correlator replay without a GPU: the numpy contract (tests/replay_spec.py) against the reference's own
correlator outputs, the exact host recurrence sgx_replay_state against the contract's state, and the shape of the
correlation peak on a noiseless record.  CPU only."""
import numpy as np
import pytest

import replay_cases as cases
import replay_spec as spec
from conftest import pkg
from oracle import softgnss_oracle as orc

DT_CODE = {"int8": 0, "<i2": 1, "uint8": 2}


def _all_cases(default_record):
    return [("default", cases.case_default(default_record)), ("rate2", cases.case_rate2())] + \
           [("int16_%d" % i, c) for i, c in enumerate(cases.cases_int16())]


@pytest.fixture(scope="module")
def golden_cases(default_record):
    return _all_cases(default_record)


def test_contract_reproduces_the_reference_arms_bit_for_bit(golden_cases):
    """Taps (-spacing, 0, +spacing) from ONLY the recorded absoluteSample / codeFreq / carrFreq and the channel's start
    equal the reference's I_E .. Q_L with np.array_equal: 4 x 400 ms, the second front end, both int16 cases."""
    for name, (s, rec, dt, chans, series) in golden_cases:
        d = s.dllCorrelatorSpacing
        out, _ = spec.replay_channels(s, rec, dt, chans, series, None, (-d, 0.0, d))
        want = cases.arms(series)
        assert out.shape == want.shape
        for c in range(len(chans)):
            for j in range(3):
                for q in range(2):
                    assert np.array_equal(out[c, j, q], want[c, j, q]), (name, c, j, q)


def test_host_state_equals_the_contract_state(golden_cases):
    n = pkg("_native")
    for name, (s, rec, dt, chans, series) in golden_cases:
        _, states = spec.replay_channels(s, rec, dt, chans, series, None, (0.0,), correlate=False)
        nbytes = np.ascontiguousarray(rec).view(np.uint8).size
        got = n.replay_state(s, chans, series, data_type=DT_CODE[dt], rec_bytes=nbytes)
        assert got.shape == (len(chans), series.shape[2])
        for c, st in enumerate(states):
            for f in spec.STATE_FIELDS:
                assert np.array_equal(got[c][f], st[f]), (name, c, f)
        # a channel cut short and a channel that is off hold zeros
        done = np.array([series.shape[2] // 2] + [series.shape[2]] * (len(chans) - 1), dtype=np.int32)
        off = [(0, 0.0, 0.0)] + chans[1:]
        got = n.replay_state(s, chans, series, ms_done=done, data_type=DT_CODE[dt])
        assert not np.any(got[0]["blk"][done[0]:]) and np.array_equal(got[0]["blk"][:done[0]], states[0]["blk"][:done[0]])
        got = n.replay_state(s, off, series, data_type=DT_CODE[dt])
        assert not np.any(got[0]["blk"]) and not np.any(got[0]["start"])


def test_host_state_errors(default_record):
    n = pkg("_native")
    s, rec, dt, chans, series = cases.case_default(default_record)
    moved = np.array(series)
    moved[2, 0, 137] += 1.0                       # one absoluteSample entry moved by one sample
    with pytest.raises(n.SgxError) as e:
        n.replay_state(s, chans, moved)
    assert e.value.code == n.SGX_E_ARG and "channel 2 block 137" in str(e.value)
    with pytest.raises(ValueError):
        spec.replay_channels(s, rec, dt, chans, moved, None, (0.0,), correlate=False)
    end = int(series[:, 0, -1].max())
    assert n.replay_state(s, chans, series, rec_bytes=end).shape == (4, 400)
    with pytest.raises(n.SgxError) as e:          # a record cut short by one byte
        n.replay_state(s, chans, series, rec_bytes=end - 1)
    assert e.value.code == n.SGX_E_RANGE and "block 399" in str(e.value)
    with pytest.raises(n.SgxError) as e:          # a record that begins after a channel's first sample
        n.replay_state(s, chans, series, rec_file_offset=int(min(c[2] for c in chans)) + 1, rec_bytes=end)
    assert e.value.code == n.SGX_E_RANGE and "block 0" in str(e.value)
    for bad in (3, 4, 5, 10, 99):                 # float / wide-integer records are not replayed
        with pytest.raises(n.SgxError) as e:
            n.replay_state(s, chans, series, data_type=bad)
        assert e.value.code == n.SGX_E_ARG
    with pytest.raises(n.SgxError) as e:
        n.replay_state(s, chans, series, ms_done=[400, 401, 400, 400])
    assert e.value.code == n.SGX_E_ARG
    nan = np.array(series)
    nan[1, 1, 10] = np.nan
    with pytest.raises(n.SgxError) as e:
        n.replay_state(s, chans, nan)
    assert e.value.code == n.SGX_E_ARG and "channel 1 block 11" in str(e.value)


def test_shape_of_the_correlation_peak_on_a_noiseless_record(capsys):
    """One satellite without noise (amplitude 60, 1 234 Hz Doppler) tracked by the oracle for 300 ms and replayed at taps
    -1.5 .. 1.5 step 0.25; mean envelope over the last 100 ms, normalised.  The maximum is at tap 0, the envelope falls
    strictly from 0 to +-1, and every tap with |d| >= 1.25 lies below 65/1023 + 2/samplesPerChip (the largest C/A side
    lobe plus one sample of ceil alignment on each side).  1 - |d| itself is not asserted: after 300 ms the 2 Hz DLL still
    sits about 0.05 chips off, so the late side lies above the ideal triangle; the largest deviation is printed."""
    ms = 300
    s = orc.OracleSettings(numberOfChannels=1, msToProcess=float(ms))
    rec, ch = cases.noiseless_record(s, ms)
    out = orc.track(s, ch, rec, ms=ms)[0]
    taps = np.arange(-1.5, 1.51, 0.25)
    I, Q, _ = spec.replay(s, rec, "int8", ch["PRN"][0], ch["acquiredFreq"][0], ch["codePhase"][0], out["absoluteSample"],
                          out["codeFreq"], out["carrFreq"], ms, taps)
    for j, name_i, name_q in ((4, "I_E", "Q_E"), (6, "I_P", "Q_P"), (8, "I_L", "Q_L")):      # taps -0.5, 0, +0.5
        assert np.array_equal(I[j], out[name_i]) and np.array_equal(Q[j], out[name_q])
    env = np.sqrt(I ** 2 + Q ** 2)[:, 200:].mean(axis=1)
    env /= env.max()
    bound = 65.0 / 1023.0 + 2.0 / (s.samplingFreq / s.codeFreqBasis)
    with capsys.disabled():
        print("\nnormalised envelope at taps -1.5 .. 1.5:", np.round(env, 3))
        print("largest deviation from 1 - |d|: %.3f; far-tap bound %.3f" % (np.max(np.abs(env - np.maximum(0, 1 - np.abs(taps)))), bound))
    assert abs(bound - 0.117) < 5e-4
    assert taps[np.argmax(env)] == 0.0
    mid = int(np.argmax(env))
    assert np.all(np.diff(env[mid:mid + 5]) < 0)          # 0 -> +1
    assert np.all(np.diff(env[mid - 4:mid + 1]) > 0)      # -1 -> 0
    assert np.all(env[np.abs(taps) >= 1.25] < bound)
