"""The speculative tracking kernel (csrc/sgx_trk3.hip) on blocks that do not lie where their pass put them: the final pass's
moved route - a scalar test for the waves that hold neither end of the block, the patch of the one or two samples that
enter or leave at its first and last lane, a block start in another 16-byte window (accumulate again).

Shape: the scene of tests/trk3_moved_scene.py - 8 hand-given channels x 300 ms at 38.192 Msps, int8, code Doppler of both
signs at a level whose DLL noise moves the short and long blocks about, starts 0, 1, 14 and 15 bytes into a window for four
channels.  The oracle ALONE shows (a condition of the test, not a result of the kernel) that in each set of map waves at
least 3 blocks start a sample early, 3 a sample late, 3 are a sample short, 3 a sample long, 3 are both and 3 start in
another window than predicted.  Each environment is one fresh child process (tests/trk3_moved_child.py) with its own
timeout; the children and the oracle run once per session.  Run with -m gpu.

Three references: the numpy oracle on the same record at test_gpu_parity.py's bars; SGX_TRK_V3=0 (trk2_kernel, which does
not speculate) at the same bars; and, array for array, tests/golden/trk3_moved_parent.npz - the series the commit BEFORE the
moved route was restructured produced for this scene on an MI355X (headline text, generic text, and the generic text on the
uint8 copy of the record, which is also held against the oracle run on that copy): the restructuring changed how the route
decides, not what it computes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden, pkg

import trk3_moved_scene as sc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("SGX_TRK3_GENERIC", "SGX_TRK_PROFILE", "SGX_TRK_TEST_SCATTER", "SGX_TRK_FASTX", "SGX_TRK_V3", "SGX_TRK_SPLIT",
            "SGX_TRK_ARMS", "SGX_TRK_STREAM", "SGX_LIB")
ENVS = {
    "plain": ({}, ("int8", "uint8")),                   # the headline text; the uint8 copy runs the generic text
    "generic": ({"SGX_TRK3_GENERIC": "1"}, ("int8",)),
    "v3off": ({"SGX_TRK_V3": "0"}, ("int8",)),          # trk2_kernel: the map on the chain, nothing predicted
}


@pytest.fixture(scope="session")
def runs(tmp_path_factory):
    """{environment name: the child's arrays}"""
    d = tmp_path_factory.mktemp("trk3_moved")
    got = {}
    for name, (env, cases) in ENVS.items():
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        e.update(env)
        path = str(d / (name + ".npz"))
        r = subprocess.run([sys.executable, os.path.join(HERE, "trk3_moved_child.py"), path] + list(cases), env=e,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, (name, r.stderr.decode(errors="replace")[-2000:])
        with np.load(path) as z:
            got[name] = {k: z[k] for k in z.files}
    return got


@pytest.fixture(scope="session")
def oracle():
    return sc.oracle_series(pkg("synth"))


@pytest.fixture(scope="session")
def oracle_uint8():
    """The oracle on the offset-binary copy of the record (a DC of 128 the correlation does not cancel to the bars'
    precision: the int8 oracle is no reference for it)."""
    from oracle import softgnss_oracle as orc
    rec = sc.record(pkg("synth"))
    ru = (rec.astype(np.int16) + 128).astype(np.uint8)
    so = orc.OracleSettings(numberOfChannels=8, msToProcess=float(sc.MS), dataType="uint8")
    chans = sc.channels()
    ch = dict(PRN=np.array([c[0] for c in chans]), acquiredFreq=np.array([c[1] for c in chans]),
              codePhase=np.array([c[2] for c in chans]), status=np.array(["T"] * 8))
    return orc.stack_series(orc.track(so, ch, ru))


def _bars(got, want, what):
    """test_gpu_parity.py's bars; every figure printed before it is asserted."""
    assert got.shape == want.shape == (8, 13, sc.MS), (what, got.shape)
    corr = max(float(np.max(np.abs(got[c, 3:9] - want[c, 3:9]))) / max(1.0, float(np.sqrt(np.mean(want[c, 3] ** 2 + want[c, 7] ** 2))))
               for c in range(8))
    cf, wf = float(np.max(np.abs(got[:, 1] - want[:, 1]))), float(np.max(np.abs(got[:, 2] - want[:, 2])))
    dd = float(np.max(np.abs(got[:, 9:13] - want[:, 9:13])))
    print("%s: absoluteSample equal %s, correlators %.3e, codeFreq %.3e Hz, carrFreq %.3e Hz, discriminators %.3e"
          % (what, np.array_equal(got[:, 0], want[:, 0]), corr, cf, wf, dd))
    assert np.array_equal(got[:, 0], want[:, 0]), what      # absoluteSample exact
    assert corr < 1e-6, (what, corr)                          # correlators, of max(1, RMS|P|)
    assert cf < 1e-6 and wf < 1e-5, (what, cf, wf)            # codeFreq, carrFreq, Hz
    assert dd < 1e-7, (what, dd)                              # discriminators / NCO commands


def test_the_scene_holds_every_class_of_moved_block_in_each_set(oracle):
    n = sc.class_counts(oracle)
    print(n)
    for c in sc.CLASSES:
        assert min(n[c]) >= sc.MIN_PER_CLASS, (c, n[c])


@pytest.mark.parametrize("env", ["plain", "generic"])
def test_moved_blocks_against_the_oracle(runs, oracle, env):
    got = runs[env]
    assert np.all(got["int8_done"] == sc.MS) and got["int8_info"][0] == 5 and got["int8_info"][1] == 20, got["int8_info"]
    _bars(got["int8"], oracle, env + " against the oracle")


def test_moved_blocks_against_the_kernel_that_does_not_speculate(runs, oracle):
    v = runs["v3off"]
    assert np.all(v["int8_done"] == sc.MS) and v["int8_info"][0] == 2, v["int8_info"]      # trk2_kernel ran
    _bars(v["int8"], oracle, "SGX_TRK_V3=0 against the oracle")
    _bars(runs["plain"]["int8"], v["int8"], "headline text against SGX_TRK_V3=0")
    _bars(runs["generic"]["int8"], v["int8"], "generic text against SGX_TRK_V3=0")


def test_moved_blocks_of_a_uint8_record_against_the_oracle(runs, oracle_uint8):
    got = runs["plain"]
    assert np.all(got["uint8_done"] == sc.MS) and got["uint8_info"][0] == 5 and got["uint8_info"][1] == 20, got["uint8_info"]
    _bars(got["uint8"], oracle_uint8, "uint8 copy against the oracle on it")


@pytest.mark.parametrize("env,case,key", [("plain", "int8", "headline"), ("generic", "int8", "generic"), ("plain", "uint8", "uint8")])
def test_moved_blocks_equal_the_parent_commits_series(runs, env, case, key):
    """Array for array, no tolerance: what the kernel computed before the moved route was restructured."""
    want = load_golden("trk3_moved_parent.npz")[key]
    got = runs[env][case]
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), (key, np.argwhere(got != want)[:4])
