"""Time the coherent multi-millisecond acquisition (sgx_acquire_coherent) on one GPU: 32 PRNs, 10 ms x 10 windows
summed non-coherently, 50 Hz bins over the default 14 kHz band, on a 100-ms window of the default synthetic scene.
Prints one JSON line: device time per call (sgx_get_timing) and wall clock, min / median over --reps calls, and the
detections of the last call.

    python tools/coherent_acq_probe.py [--reps 10] [--coherent-ms 10] [--windows 10] [--step 50]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--coherent-ms", type=int, default=10)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--step", type=float, default=50.0)
    ap.add_argument("--coherent-rule", action="store_true", help="keep the larger window instead of summing")
    a = ap.parse_args()
    importlib.import_module("__graft_entry__").build()
    m = importlib.import_module("softgnss-python_amd")
    s = m.Settings()
    n = s.samplesPerCode
    ms = max(11, a.coherent_ms * a.windows) + 1
    ctx = m.engine.get_context(s, 0)
    rec = ctx.synth(m.synth.Scene.default(), m.synth.record_length(n, ms))
    kw = dict(coherent_ms=a.coherent_ms, n_windows=a.windows, noncoh=not a.coherent_rule, bin_step_hz=a.step)
    plan = m._native.acquire_coherent_plan(s, **kw)
    dev, wall = [], []
    r = None
    for i in range(a.reps + 1):
        t0 = time.perf_counter()
        r = ctx.acquire_coherent(rec, 0, ms * n, list(range(32)), **kw)
        t1 = time.perf_counter()
        if i:   # (the first call allocates and plans)
            wall.append((t1 - t0) * 1e3)
            dev.append(ctx.timing()["acquire_ms"])
    rec.free()
    print(json.dumps(dict(kind="coherent_acq", plan=plan, params=kw, reps=a.reps,
                          device_ms_min=min(dev), device_ms_median=float(np.median(dev)),
                          wall_ms_min=min(wall), wall_ms_median=float(np.median(wall)),
                          detected=[int(p) + 1 for p in np.flatnonzero(r["carrFreq"] > 0)])))


if __name__ == "__main__":
    main()
