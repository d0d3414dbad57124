"""The moved route of the speculative tracking kernel's final pass (csrc/sgx_trk3.hip: t3_map_role), without a GPU:

* the numpy restatement of the pass's block predictor (tests/trk3_moved_scene.py: two `advance` steps with the older block's
  code rate) on the ORACLE's series of the moved-block scene - how far a block can lie from where its pass put it, and that
  the scene holds every class of moved block in each set of map waves often enough for tests/test_trk3_moved_blocks_gpu.py;
* the texts the build makes of the kernel: restructuring the moved route must leave the plain route - every instruction
  from the final pass's `s_setprio 2` to the `s_setprio 0` behind the publish - what it was (tests/golden/
  trk3_plain_route.txt: the sequence of the commit before the change, register numbers and labels taken out), spill no
  vector register, touch v[244:255] nowhere outside the polls, and spill no more scalar registers than before (44 in the
  headline text, 46 in the generic one)."""
import os
import re
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, pkg

import trk3_moved_scene as sc

SGPR_SPILLS_BEFORE = {"T3Headline": 44, "T3Generic": 46}


@pytest.fixture(scope="module")
def oracle():
    return sc.oracle_series(pkg("synth"))


def test_predictor_restated_in_numpy_against_the_oracle(oracle):
    """A block's start is off by what the length of the block before it was mispredicted by, with a rate one block old: at
    most one sample (the DLL moves the code rate by less than 27 Hz per block: 2.6e-5 of 38 192 samples); its length by the
    phase two rate steps leave: at most two.  The series' own lengths follow from the carried code phase (block_table
    asserts tracking.py:148 block by block), so the restatement carries it as the reference does."""
    exact = total = 0
    for ch, (_, _, phase) in enumerate(sc.channels()):
        start, blk, step, rem = sc.block_table(oracle[ch], phase)
        assert np.all(np.abs(blk - 38192) <= 1) and np.all(rem[1:] > -1e-9) and np.all(rem < step + 1e-9)
        ps, pl = sc.predicted(start, blk, step, rem)
        ds, dl = (start - ps)[2:], (blk - pl)[2:]
        assert np.all(np.abs(ds) <= 1) and np.all(np.abs(dl) <= 2), (ch, ds.min(), ds.max(), dl.min(), dl.max())
        exact += int(np.sum((ds == 0) & (dl == 0)))
        total += ds.size
        # the starts of the first four channels lie at a window's edge: 0, 1, 14, 15 bytes into it
        if ch < 4:
            assert int(start[0]) & 15 == (0, 1, 14, 15)[ch]
    print("%d of %d blocks lie where their pass put them" % (exact, total))
    assert 0.5 * total < exact < 0.97 * total      # (predictions flip often here: 3 % of the blocks in the default scene)


def test_the_scene_holds_every_class_of_moved_block_in_each_set(oracle):
    n = sc.class_counts(oracle)
    print(n)
    for c in sc.CLASSES:
        assert min(n[c]) >= sc.MIN_PER_CLASS, (c, n[c])


def _normalised(t):
    t = re.sub(r"\b([vsa])\[\d+:\d+\]", r"\1[]", t)
    t = re.sub(r"\b([vs])\d+\b", r"\1", t)
    return re.sub(r"\.LBB\d+_\d+", "L", t)


def test_the_kernel_texts_keep_the_plain_route_and_their_registers():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    b = pkg("build")
    ok, msg = b.check_trk3_registers((), hipcc)          # v[244:255] outside the polls, vector spills, AGPRs: every kernel
    assert ok, msg
    ok, text = b.trk3_assembly((), hipcc)
    assert ok, text
    kernels = b.trk3_kernels(text)
    assert len(kernels) == 2, sorted(kernels)
    for case, before in SGPR_SPILLS_BEFORE.items():
        (name,) = [k for k in kernels if case in k]
        meta = kernels[name]["meta"]
        print(case, "sgpr spills", meta[".sgpr_spill_count"], "instructions", len(kernels[name]["body"]))
        assert int(meta[".vgpr_spill_count"]) == 0, (case, meta[".vgpr_spill_count"])
        assert int(meta[".sgpr_spill_count"]) <= before, (case, meta[".sgpr_spill_count"])
    # the plain route of the headline text: the first s_setprio 2 of the kernel is the final pass's, the next s_setprio 0 the
    # one behind the publish; the routes off the plain one are blocks placed elsewhere and reached by branches
    (name,) = [k for k in kernels if "T3Headline" in k]
    body = kernels[name]["body"]
    i = body.index("s_setprio 2")
    j = body.index("s_setprio 0", i)
    got = [_normalised(t) for t in body[i:j + 1]]
    with open(os.path.join(GOLDEN, "trk3_plain_route.txt")) as f:
        want = f.read().split("\n")[:-1]
    assert len(want) > 100
    assert got == want, [(k, a, c) for k, (a, c) in enumerate(zip(got, want)) if a != c][:5] or (len(got), len(want))
