"""Time one sgx_track_quality call (C/N0 + lock detector, csrc/sgx_quality.hip) for 8 channels x 37 000 ms and for
3 072 channels x 500 ms, and print the per-window C/N0 / carrier-lock spread behind Settings' lock-detector defaults:
the default scene's channels over 37 s, and channels on PRNs absent from the scene (noise only).
Usage (GPU box): python tools/quality_probe.py [out.json]"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
m = importlib.import_module("softgnss-python_amd")


def timed(ctx, i_p, q_p, p, reps=20):
    ctx.track_quality(i_p, q_p, p)                  # warm-up: code object, allocation sizes
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.track_quality(i_p, q_p, p)
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), reps=reps)


def main():
    s = m.Settings()
    ctx = m.engine.get_context(s, 0)
    p = m._native.lock_params(s)
    sc = m.synth.Scene.default()
    rec = ctx.synth(sc, m.synth.record_length(s.samplesPerCode, 37000))
    a = m.AcquisitionResult(s, device=0)
    a.acquire(m.DeviceSignal(rec, 0, 11 * s.samplesPerCode))
    a.preRun()
    t = m.TrackingResult(a, device=0)
    t.track(m.DeviceFile(rec))
    series = t.series                                 # pinned [8, 13, 37000]
    out = {"8x37000_strided_pinned": timed(ctx, series[:, 3], series[:, 7], p),
           "8x37000_contiguous_pageable": timed(ctx, np.ascontiguousarray(series[:, 3]),
                                                np.ascontiguousarray(series[:, 7]), p)}
    big_i = m._native.pinned_empty((3072, 500))
    big_q = m._native.pinned_empty((3072, 500))
    big_i[:] = np.tile(series[:, 3, 1000:1500], (384, 1))
    big_q[:] = np.tile(series[:, 7, 1000:1500], (384, 1))
    out["3072x500_contiguous_pinned"] = timed(ctx, big_i, big_q, p)
    out["3072x500_contiguous_pageable"] = timed(ctx, np.array(big_i), np.array(big_q), p)
    # the spread behind the defaults: the default scene over 37 s ...
    cno, cl, ok, lost = ctx.track_quality(series[:, 3], series[:, 7], p)
    sig = {}
    for j, c in enumerate(a.channels):
        x, y = cno[j, 5:], cl[j, 5:]                     # after the first 100 ms of pull-in
        sig[int(c.PRN)] = dict(cno_p1_p50_p99=[float(v) for v in np.percentile(x, [1, 50, 99])],
                               carr_p1_p50=[float(v) for v in np.percentile(y, [1, 50])],
                               pass_frac=float(np.mean(ok[j])), lost=int(lost[j]))
    out["scene_windows"] = sig
    # ... and noise-only channels (PRNs absent from the scene, various frequency errors)
    absent = [p_ for p_ in range(1, 33) if p_ not in [x["prn"] for x in sc.sats]][:16]
    chans = [(prn, s.IF + 500.0 * (k - 8), 1000.0 * k + 17.0) for k, prn in enumerate(absent)]
    ns, done = ctx.track(rec, chans, 4000)
    cno, cl, ok, lost = ctx.track_quality(ns[:, 3], ns[:, 7], p)
    out["noise_windows"] = dict(cno_p50_p90_p99=[float(v) for v in np.percentile(cno, [50, 90, 99])],
                                carr_p50_p90=[float(v) for v in np.percentile(cl, [50, 90])],
                                pass_frac=float(np.mean(ok)), lost_at_ms=[int((v + 1) * p.window) for v in lost])
    rec.free()
    print(json.dumps(out, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
