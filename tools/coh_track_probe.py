"""Kernel time per block of sgx_track_coherent (csrc/sgx_trk_coh.hip) on one GPU, next to sgx_track on the same record and
channels:

    python tools/coh_track_probe.py [--calls 10] [--ms 4000]

Three configurations of 8 channels x --ms blocks: the default 38.192 Msps scene at T = 20 (pull-in 1 000 ms, the bit
edges found), the same with the pull-in as long as the run (every update a 1 ms update), and a 4.092 Msps scene at T = 20.
One warm-up call, then --calls timed calls of each entry point; HIP events around the kernel on the context's stream
(sgx_get_timing's track_ms).  Prints one JSON line per configuration: min and median kernel ms, the same per block and
channel in microseconds, sgx_track's figures with the kernel it chose, and the ratio of the minima."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, ctx, calls):
    out = []
    for i in range(calls + 1):
        call()
        if i:
            out.append(ctx.timing()["track_ms"])
    return out, ctx.timing()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--ms", type=int, default=4000)
    a = ap.parse_args()
    m = importlib.import_module("softgnss-python_amd")
    n_ = m._native
    ms = a.ms
    for name, fs, IF, pull_in in (("default scene, T=20", 38192000.0, 9548000.0, min(1000, ms)),
                                  ("default scene, all 1 ms updates", 38192000.0, 9548000.0, ms),
                                  ("4.092 Msps, T=20", 4092000.0, 1000000.0, min(1000, ms))):
        s = m.Settings()
        s.samplingFreq, s.IF, s.msToProcess = fs, IF, float(ms)
        ctx = m.engine.get_context(s, 0)
        n = s.samplesPerCode
        rec = ctx.synth(m.synth.Scene.default(fs, IF), m.synth.record_length(n, ms))
        acq = m.AcquisitionResult(s, device=0)
        acq.acquire(m.DeviceSignal(rec, 0, 11 * n))
        acq.preRun()
        chans = [(int(c.PRN), float(c.acquiredFreq), float(c.codePhase)) for c in acq.channels if c.PRN != 0]
        params = n_.coh_params(s, 20, pull_in, 100)
        got = ctx.track_coherent(rec, chans, ms, params)
        assert np.all(got[1] == ms)
        coh, _ = timed(lambda: ctx.track_coherent(rec, chans, ms, params), ctx, a.calls)
        ref, tim = timed(lambda: ctx.track(rec, chans, ms), ctx, a.calls)
        per = 1e3 / ms                                     # ms per call -> us per block (the channels run side by side)
        print(json.dumps(dict(case=name, channels=len(chans), ms=ms, samples_per_code=n, pull_in_ms=pull_in, calls=a.calls,
                              bit_edges=[int(e) for e in got[2]], coherent_start=[int(k) for k in got[3]],
                              coherent_ms_min=round(min(coh), 3), coherent_ms_median=round(float(np.median(coh)), 3),
                              coherent_us_per_block_min=round(min(coh) * per, 3),
                              coherent_us_per_block_median=round(float(np.median(coh)) * per, 3),
                              track_ms_min=round(min(ref), 3), track_ms_median=round(float(np.median(ref)), 3),
                              track_us_per_block_min=round(min(ref) * per, 3),
                              track_us_per_block_median=round(float(np.median(ref)) * per, 3),
                              track_kernel=tim["track_kernel"], track_members=tim["track_members"],
                              ratio_of_minima=round(min(coh) / min(ref), 2))), flush=True)
        rec.free()


if __name__ == "__main__":
    main()
