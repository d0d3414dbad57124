"""Child process of tests/test_coherent_acq_gpu.py: one dense case (tests/dense_scene.py) searched on the GPU in a fresh
process, whose environment the parent chose (SGX_ACQ_FINE_V1), results saved as .npz.  argv: case name, output path."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def run_case(m, c):
    """The library's search of a dense case: dict of the five outputs in the order of c.prns."""
    s = m.Settings()
    s.samplingFreq, s.IF, s.acqSearchBand = c.s.samplingFreq, c.s.IF, c.s.acqSearchBand
    ctx = m.engine.get_context(s, 0)
    kw = dict(coherent_ms=c.T, n_windows=c.M, noncoh=c.noncoh, bin_step_hz=c.step)
    if c.f64:
        return ctx.acquire_coherent_f64(c.signal().astype(np.float64), c.prns, **kw)
    rec = ctx.upload(c.record())
    try:
        return ctx.acquire_coherent(rec, c.offset, c.n_samples, c.prns, **kw)
    finally:
        rec.free()


if __name__ == "__main__":
    import importlib
    import dense_scene
    got = run_case(importlib.import_module("softgnss-python_amd"), dense_scene.BY_NAME[sys.argv[1]])
    np.savez(sys.argv[2], **got)
