"""The speculative tracking kernel's instantiations (csrc/sgx_trk3.hip: T3Headline, T3Generic) against each other and against
the reference's goldens.  What a launch is - int8 or offset-binary samples, a resident or a streaming record, the profile on or
off, the members of a channel on one XCD or not - selects a kernel TEXT, never a result: every series must equal the run of
the generic text (SGX_TRK3_GENERIC=1) array for array, with no tolerance.

Shape: 8 channels x 60 ms at 38.192 Msps on the default scene - block 0's direct path, the pull-in blocks that accumulate
again, patched blocks - plus 3 channels (a launch padded to eight) and ms = 1.  Each environment is one fresh child
process (tests/trk3_cases_child.py) with its own timeout; the children run once per session.  Run with -m gpu.

The anchor is the reference's output, not the other instantiation: the headline text tracks the channel table of
tests/golden/trk_default.npz (the reference's own 400-ms run; its first 60 ms here) to the bars of test_gpu_parity.py
(absoluteSample exact, correlators within 1e-6 of max(1, RMS|P|)), and a record that ends inside the run as
tests/golden/trk_short.npz records the reference doing (None returned, results unset, file closed)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TRK_TOL = 1e-6      # test_gpu_parity.py's bar for the correlator series
SWITCHES = ("SGX_TRK3_GENERIC", "SGX_TRK_PROFILE", "SGX_TRK_TEST_SCATTER", "SGX_TRK_FASTX", "SGX_TRK_V3", "SGX_TRK_SPLIT",
            "SGX_TRK_ARMS", "SGX_TRK_STREAM", "SGX_LIB")
ENVS = {
    "plain": ({}, ()),                                             # every case, each with the text the launch site picks
    "generic": ({"SGX_TRK3_GENERIC": "1"}, ()),                    # ... with the generic text
    "profile": ({"SGX_TRK_PROFILE": "1"}, ("int8",)),
    "scatter": ({"SGX_TRK_TEST_SCATTER": "1"}, ("int8", "ch3")),   # the headline text told its members are scattered
}


@pytest.fixture(scope="session")
def runs(tmp_path_factory):
    """{environment name: (the child's arrays, its stderr)}"""
    d = tmp_path_factory.mktemp("trk3_cases")
    got = {}
    for name, (env, cases) in ENVS.items():
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        e.update(env)
        path = str(d / (name + ".npz"))
        r = subprocess.run([sys.executable, os.path.join(HERE, "trk3_cases_child.py"), path] + list(cases), env=e,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, (name, r.stderr.decode(errors="replace")[-2000:])
        with np.load(path) as z:
            got[name] = ({k: z[k] for k in z.files}, r.stderr.decode(errors="replace"))
    return got


def _same(a, b, case):
    assert np.array_equal(a[case + "_done"], b[case + "_done"]), case
    assert a[case].shape == b[case].shape and np.array_equal(a[case], b[case]), (case, np.argwhere(a[case] != b[case])[:4])


@pytest.mark.parametrize("case", ["int8", "uint8", "stream", "ch3", "ms1"])
def test_the_launch_sites_text_equals_the_generic_text(runs, case):
    """int8 resident (the headline text), uint8 and a record streaming in from a file (the generic text either way), three
    channels in a launch padded to eight and a single block: bit for bit the generic text's series."""
    plain, generic = runs["plain"][0], runs["generic"][0]
    ms = 1 if case == "ms1" else 60
    assert plain[case].shape == (3 if case == "ch3" else 8, 13, ms) and np.all(plain[case + "_done"] == ms)
    assert plain[case + "_info"][0] == 5 and plain[case + "_info"][1] == 20, plain[case + "_info"]   # trk3_kernel, 20 members
    assert generic[case + "_info"][0] == 5 and generic[case + "_info"][1] == 20
    _same(plain, generic, case)
    if case == "stream":   # the way the samples arrive changes nothing (test_streaming_record_overlaps_tracking_...)
        assert np.array_equal(plain[case], generic["int8"])


def test_profile_run_equals_the_generic_text(runs):
    """SGX_TRK_PROFILE=1 (the generic text with the profile buffer) leaves the series what they are and prints its lines."""
    prof, err = runs["profile"]
    _same(prof, runs["generic"][0], "int8")
    assert "[sgx trk2 profile] ch 0 member  0 cycles/block" in err


def test_headline_text_stops_for_scattered_members_and_the_launch_is_repeated(runs):
    """The headline text takes a channel's members to share an XCD; told otherwise (the test hook) every channel stops before
    block 0, the host says so and repeats the launch with the generic text: the same series."""
    got, err = runs["scatter"]
    for case in ("int8", "ch3"):
        _same(got, runs["generic"][0], case)
        assert got[case + "_info"][0] == 5 and got[case + "_info"][1] == 20
    assert err.count("do not share an XCD; repeating the launch") == 2
    assert "do not share an XCD" not in runs["plain"][1]


def test_headline_text_against_the_reference_goldens(runs):
    g = load_golden("trk_default.npz")
    gs = load_golden("trk_short.npz")
    plain = runs["plain"][0]
    got, want = plain["golden4"], g["series"][:, :, :60]
    assert got.shape == want.shape and np.all(plain["golden4_done"] == 60)
    assert np.array_equal(got[:, 0], want[:, 0])                     # absoluteSample bit-exact
    for c in range(4):
        scale = max(1.0, float(np.sqrt(np.mean(want[c, 3] ** 2 + want[c, 7] ** 2))))
        assert np.max(np.abs(got[c, 3:9] - want[c, 3:9])) / scale < TRK_TOL
    assert np.max(np.abs(got[:, 1] - want[:, 1])) < 1e-6             # codeFreq, Hz
    assert np.max(np.abs(got[:, 2] - want[:, 2])) < 1e-5             # carrFreq, Hz
    assert np.max(np.abs(got[:, 9:13] - want[:, 9:13])) < 1e-7       # discriminators / NCO commands
    _same(plain, runs["generic"][0], "golden4")
    # a record of trk_short.npz's length: what the reference did with it
    assert bool(gs["returned_none"]) and bool(gs["results_unset"]) and bool(gs["closed"])
    assert list(plain["short"]) == [True, True, True] and list(runs["generic"][0]["short"]) == [True, True, True]
