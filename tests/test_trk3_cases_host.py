"""The texts of the speculative tracking kernel's instantiations (csrc/sgx_trk3.hip: T3Headline, T3Generic), as the build
compiles them to assembly (softgnss-python_amd/build.py: trk3_assembly, the register gate's own compile).  No GPU needed."""
import os
import re
import shutil

import pytest

from conftest import pkg

PROF_ARG = 6       # trk3_kernel(rec, codes, chans, out, ms_done, K, prof, xch, err)


def _kernarg_loads(body):
    """[(first byte, one past the last byte)] of the kernel-argument segment that the scalar loads of `body` read: loads
    through s[0:1] (the segment's address) or through a register pair made of it by s_add_u32 / s_addc_u32 with a constant."""
    base = {"0": 0}            # low register of a pair -> byte offset of the pair's address in the segment
    spans = []
    for t in body:
        m = re.match(r"s_add_u32 s(\d+), s0, (0x[0-9a-f]+|\d+)$", t)
        if m:
            base[m.group(1)] = int(m.group(2), 0)
            continue
        m = re.match(r"s_load_dword(x(\d+))? \S+, s\[(\d+):\d+\], (0x[0-9a-f]+|\d+)", t)
        if m and m.group(3) in base:
            lo = base[m.group(3)] + int(m.group(4), 0)
            spans.append((lo, lo + 4 * int(m.group(2) or 1)))
    return spans


def test_every_instantiation_passes_the_gate_and_the_headline_text_never_reads_the_profile_buffer():
    """Three things about the texts the build makes: the register gate holds (v[244:255] only inside the polls, over the
    whole file; no kernel of it spills a vector register or uses AGPRs); every instantiation keeps 0 bytes of scratch and
    at most 256 VGPRs; and the headline text holds no load of the profile buffer's kernel argument, which the generic text
    does load (the same scan finds it there)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    b = pkg("build")
    ok, msg = b.check_trk3_registers((), hipcc)
    assert ok, msg
    ok, text = b.trk3_assembly((), hipcc)
    assert ok, text
    kernels = b.trk3_kernels(text)
    head = [k for k in kernels if "T3Headline" in k]
    gen = [k for k in kernels if "T3Generic" in k]
    assert len(kernels) == 2 and len(head) == 1 and len(gen) == 1, sorted(kernels)
    assert "no spills in 2 kernels" in msg, msg      # (the gate looked at each of them)
    for name, k in kernels.items():
        meta = k["meta"]
        assert int(meta[".private_segment_fixed_size"]) == 0, (name, meta[".private_segment_fixed_size"])
        assert int(meta[".vgpr_spill_count"]) == 0 and int(meta[".agpr_count"]) == 0, name
        assert int(meta[".vgpr_count"]) <= 256, (name, meta[".vgpr_count"])
        assert len(k["args"]) >= 9 and len(k["body"]) > 1000, name
    spans = {}
    for name in head + gen:
        k = kernels[name]
        lo, size = int(k["args"][PROF_ARG][".offset"]), int(k["args"][PROF_ARG][".size"])
        assert size == 8 and k["args"][PROF_ARG][".value_kind"] == "global_buffer"
        loads = _kernarg_loads(k["body"])
        assert len(loads) >= 6, (name, loads)         # (the scan finds the kernel's argument loads)
        spans[name] = [s for s in loads if s[0] < lo + size and s[1] > lo]
    assert spans[gen[0]], "the generic text must load the profile buffer's pointer (or this scan does not see such loads)"
    assert not spans[head[0]], spans[head[0]]
    # ... and it is the shorter text: the tests and the branches of the other cases are not in it
    assert len(kernels[head[0]]["body"]) < len(kernels[gen[0]]["body"])
