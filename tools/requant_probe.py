"""Times of the requantiser's two kernels (csrc/sgx_requant.hip: the statistics pass of sgx_requant_stats_of and the
quantiser of sgx_if_requantize) on one GPU:

    python tools/requant_probe.py [--ms 37000] [--calls 10]

The record is the default scene of --ms code periods (37 000: the 1.4 GB record of the benchmark), its bytes read as int16
and as float32 elements (every bit pattern is a legal element; the float view holds NaNs and denormals, which cost what
any other value costs).  One warm-up call, then --calls timed calls per kernel and type; HIP events on the context's stream
around the kernel.  Prints one JSON line with the read and copy rates sgx_stream_rates measures on the same GPU, then one
line per kernel and type: min and median in ms beside the floor - bytes read / read rate for the statistics pass, (bytes
read + written) / copy rate for the quantiser - and the share of the floor's rate the kernel reaches."""
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
    ctx = m.engine.get_context(s, 0)
    n = m.synth.record_length(s.samplesPerCode, a.ms)
    rec = ctx.synth(m.synth.Scene.default(), n - n % 4)
    read_gbs, copy_gbs = ctx.stream_rates()
    print(json.dumps(dict(bytes=len(rec), read_GBps=round(read_gbs, 1), copy_GBps=round(copy_gbs, 1))), flush=True)
    for dtype, w, gain in (("int16", 2, dict(mult=24969, shift=20)), ("float32", 4, dict(scale=24512.5))):
        st_ms, q_ms = [], []
        for i in range(a.calls + 1):
            ctx.requant_stats(rec, dtype)
            out = ctx.requantize(rec, dtype, **gain)
            out.free()
            if i:
                t = ctx.requant_timing()
                st_ms.append(t[0])
                q_ms.append(t[1])
        moved = len(rec) + len(rec) // w
        for kernel, ms, floor in (("requant_stats_kernel", st_ms, len(rec) / read_gbs / 1e6),
                                  ("requant_kernel", q_ms, moved / copy_gbs / 1e6)):
            print(json.dumps(dict(kernel=kernel, dtype=dtype, calls=a.calls, kernel_ms_min=round(min(ms), 3),
                                  kernel_ms_median=round(float(np.median(ms)), 3), floor_ms=round(floor, 3),
                                  share_of_floor_rate=round(floor / min(ms), 3))), flush=True)
    rec.free()


if __name__ == "__main__":
    main()
