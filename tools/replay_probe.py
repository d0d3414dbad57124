"""Time of sgx_track_replay (the multi-correlator replay, csrc/sgx_replay.hip) on one GPU:

    python tools/replay_probe.py --case config3 [--calls 10]    8 channels x 37 000 ms, K = 3, 11, 41 taps, next to the
                                                                tracking launch that produced the series (track_ms)
    python tools/replay_probe.py --case many [--calls 10]       3 072 channels x 500 ms, K = 11

One warm-up call, then --calls timed calls; HIP events on the context's stream: the kernel alone and the whole device
side (state upload, kernel, result copy).  Prints one JSON line per measurement: min and median in ms, and the
algorithmic rate (the record bytes the blocks cover, read once) against the 8 TB/s HBM peak.  Run each case as its own
process, under its own time limit."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def measure(ctx, rec, chans, series, taps, calls):
    ker, dev = [], []
    for i in range(calls + 1):
        ctx.track_replay(rec, chans, series, taps)
        k, d = ctx.replay_timing()
        if i:
            ker.append(k)
            dev.append(d)
    return ker, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("config3", "many"), required=True)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    m = importlib.import_module("softgnss-python_amd")
    s = m.Settings()
    ms = 37000 if a.case == "config3" else 500
    s.msToProcess = float(ms)
    ctx = m.engine.get_context(s, 0)
    n = s.samplesPerCode
    rec = ctx.synth(m.synth.Scene.default(), m.synth.record_length(n, 37000 if a.case == "config3" else 500 + 384 + 1))
    acq = m.AcquisitionResult(s, device=0)
    acq.acquire(m.DeviceSignal(rec, 0, 11 * n))
    acq.preRun()
    chans = [(int(c.PRN), float(c.acquiredFreq), float(c.codePhase)) for c in acq.channels if c.PRN != 0]
    if a.case == "many":
        chans = [(chans[i % 8][0], chans[i % 8][1], chans[i % 8][2] + (i // 8) * n) for i in range(3072)]
    series, done = ctx.track(rec, chans, ms)
    assert np.all(done == ms)
    tim = ctx.timing()
    spacing = float(s.dllCorrelatorSpacing)
    banks = {3: [-spacing, 0.0, spacing], 11: list(np.linspace(-1.25, 1.25, 11)), 41: list(np.linspace(-2.0, 2.0, 41))}
    nbytes = float(np.sum(series[:, 0, -1] - np.array([s.skipNumberOfBytes + c[2] for c in chans])))
    for K in ((3, 11, 41) if a.case == "config3" else (11,)):
        ker, dev = measure(ctx, rec, chans, series, banks[K], a.calls)
        if K == 3:
            got = ctx.track_replay(rec, chans, series, banks[3])
            err = max(float(np.max(np.abs(got[c, :, 0] - series[c, [4, 3, 5]]))) /
                      max(1.0, float(np.sqrt(np.mean(series[c, 3] ** 2 + series[c, 7] ** 2)))) for c in range(len(chans)))
        else:
            err = None
        print(json.dumps(dict(case=a.case, channels=len(chans), ms=ms, taps=K, calls=a.calls,
                              track_ms=round(tim["track_ms"], 3), track_kernel=tim["track_kernel"],
                              kernel_ms_min=round(min(ker), 3), kernel_ms_median=round(float(np.median(ker)), 3),
                              device_ms_min=round(min(dev), 3), device_ms_median=round(float(np.median(dev)), 3),
                              record_gb=round(nbytes / 1e9, 3), gbps=round(nbytes / (min(ker) * 1e-3) / 1e9, 1),
                              hbm_peak_fraction=round(nbytes / (min(ker) * 1e-3) / HBM_PEAK, 4),
                              err_vs_tracked_arms=err)), flush=True)
    rec.free()


if __name__ == "__main__":
    main()
