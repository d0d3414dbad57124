"""Times of the two kernels of the front-end conditioning stage (csrc/sgx_cond.hip: cond_stats_kernel of
sgx_cond_block_stats and cond_apply_kernel of sgx_if_condition) on one GPU:

    python tools/cond_probe.py [--ms 37000] [--calls 10]

The record is the default scene of --ms code periods (37 000: the 1.4 GB record of the benchmark), its bytes read as int8
samples in one lane and as interleaved int16 pairs, in blocks of 100 us (3824 frames) with blanking at 4 x the rms and a
guard of 8 frames, the defaults of Settings.  One warm-up call, then --calls timed calls per kernel and format; HIP events
on the context's stream around the kernel.  Prints one JSON line with the read and copy rates sgx_stream_rates measures on
the same GPU, then one line per kernel and format: min and median in ms beside the floor - bytes read / read rate for the
statistics kernel, (bytes read + written) / copy rate for the apply kernel - and the share of the floor's rate the kernel
reaches."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", type=int, default=37000)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    m = importlib.import_module("softgnss-python_amd")
    s = m.Settings()
    s.frontEndConditioning = True
    ctx = m.engine.get_context(s, 0)
    n = m.synth.record_length(s.samplesPerCode, a.ms)
    rec = ctx.synth(m.synth.Scene.default(), n - n % 4)
    read_gbs, copy_gbs = ctx.stream_rates()
    print(json.dumps(dict(bytes=len(rec), read_GBps=round(read_gbs, 1), copy_GBps=round(copy_gbs, 1))), flush=True)
    _, _, block, blank_q4 = s._cond_format()
    for dtype, w, lanes in (("int8", 1, 1), ("int16", 2, 2)):
        st_ms, ap_ms = [], []
        for i in range(a.calls + 1):
            stats = ctx.cond_stats(rec, dtype, lanes, block, blank_q4)
            plan = m._native.cond_plan(stats, lanes, blank_q4, s.condTargetRms, s.condAgcBlocks)
            out = ctx.condition(rec, dtype, lanes, block, plan, int(s.condGuardFrames))
            blanked, clipped = out.blanked, out.clipped
            out.free()
            if i:
                t = ctx.cond_timing()
                st_ms.append(t[0])
                ap_ms.append(t[1])
        moved = len(rec) + len(rec) // w
        for kernel, ms, floor in (("cond_stats_kernel", st_ms, len(rec) / read_gbs / 1e6),
                                  ("cond_apply_kernel", ap_ms, moved / copy_gbs / 1e6)):
            print(json.dumps(dict(kernel=kernel, dtype=dtype, lanes=lanes, block=block, blocks=int(plan.size), calls=a.calls,
                                  kernel_ms_min=round(min(ms), 3), kernel_ms_median=round(float(np.median(ms)), 3),
                                  floor_ms=round(floor, 3), share_of_floor_rate=round(floor / min(ms), 3),
                                  blanked_frames=blanked, clipped=clipped)), flush=True)
    rec.free()


if __name__ == "__main__":
    main()
