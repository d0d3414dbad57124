"""Times of the record monitor's kernels (csrc/sgx_waterfall.hip: sgx_probe_waterfall) on one GPU beside its two yardsticks:

    python tools/waterfall_probe.py [--ms 37000] [--calls 10] [--loop-calls 2]      (--loop-calls 0: no baseline)

The input is the default scene's record of --ms code periods (37 000: the 1.4 GB record of the benchmark), monitored at the
defaults (100 ms slices, segments of 16384 that share 1024).  One warm-up call, then --calls timed calls; HIP events on the
context's stream around the kernels.  Prints one JSON line with the read and copy rates sgx_stream_rates measures in the same
job and the read floor (the record's bytes at the read rate); one line with the monitor's kernel time, min and median; one
line with the same analysis done slice by slice - sgx_probe_stats called once per slice, wall clock around the loop.
sgx_probe_stats is the monitor at one slice, so the loop now measures what a call costs around the same kernels (the
launches, a synchronisation and the copies back per slice), and the largest difference between the two spectra relative
to each slice's largest bin is 0."""
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
    ap.add_argument("--ms", type=int, default=37000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--loop-calls", type=int, default=2)
    a = ap.parse_args()
    m = importlib.import_module("softgnss-python_amd")
    s = m.Settings()
    ctx = m.engine.get_context(s, 0)
    n = m.synth.record_length(s.samplesPerCode, a.ms)
    rec = ctx.synth(m.synth.Scene.default(), n)
    ctx.sync()
    read_gbs, copy_gbs = ctx.stream_rates()
    print(json.dumps(dict(in_bytes=n, read_GBps=round(read_gbs, 1), copy_GBps=round(copy_gbs, 1),
                          read_floor_ms=round(n / read_gbs / 1e6, 3))), flush=True)
    fs_mhz = s.samplingFreq / 1e6
    N, noverlap = int(s.monitorSegment), int(s.monitorOverlap)
    S = int(np.rint(s.monitorSliceMs * 1e-3 * s.samplingFreq))
    ms, wall = [], []
    for i in range(a.calls + 1):
        t0 = time.perf_counter()
        seen = ctx.waterfall(rec, 0, n, fs_mhz, N, noverlap, S)
        if i:
            wall.append(1e3 * (time.perf_counter() - t0))
            ms.append(ctx.waterfall_timing())
    segments = int(seen.n_segments.sum())
    print(json.dumps(dict(kernel="sgx_probe_waterfall", slices=len(seen.n_segments), segments=segments, calls=a.calls,
                          kernel_ms_min=round(min(ms), 3), kernel_ms_median=round(float(np.median(ms)), 3),
                          call_ms_min=round(min(wall), 3), us_per_segment=round(1e3 * min(ms) / segments, 3),
                          GBps=round(n / min(ms) / 1e6, 1))), flush=True)
    if a.loop_calls > 0 and N == 16384 and noverlap == 1024:                  # (the probe's own parameters: its loop is the same analysis)
        loop, worst = [], 0.0
        for i in range(a.loop_calls + 1):
            t0 = time.perf_counter()
            rows = [ctx.probe_stats(rec, j * S, min(S, n - j * S), fs_mhz)[1] for j in range(len(seen.n_segments))]
            if i:
                loop.append(1e3 * (time.perf_counter() - t0))
        for row, pxx in zip(rows, seen.pxx):
            worst = max(worst, float(np.abs(row - pxx).max() / pxx.max()))
        print(json.dumps(dict(baseline="sgx_probe_stats per slice", calls=a.loop_calls, loop_ms_min=round(min(loop), 3),
                              loop_ms_median=round(float(np.median(loop)), 3),
                              speedup_over_loop=round(min(loop) / min(wall), 2), max_rel_difference=worst)), flush=True)
    rec.free()


if __name__ == "__main__":
    main()
