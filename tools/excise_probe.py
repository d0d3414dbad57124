"""Time of sgx_if_excise's kernel (swept-interference excision, csrc/sgx_excise.hip) on one GPU:

    python tools/excise_probe.py [--ms 37000] [--segments 64,256,1024] [--calls 10]

The record is the default scene of --ms code periods (37 000: the 1.4 GB record of the benchmark).  One warm-up call, then
--calls timed calls; HIP events on the context's stream around the kernel.  Prints one JSON line per segment length: min and
median in ms next to two floors measured or counted in the same run -
  copy_floor_ms   the record read and written once at the copy rate of sgx_stream_rates (read + write bytes counted);
  fp64_floor_ms   the fp64 operations of the two transforms of every segment a tile computes (5 M log2 M each for the M = N / 2
                  point complex transform, S / (S - 1) of the segments for the one a tile shares with the next) at the vector
                  fp64 peak, 78.6 TFLOP/s (256 CUs x 4 SIMDs x 16 lanes x 2 per fused operation at 2.4 GHz; the kernel is
                  built without contraction, so half of that is what its separate multiplies and adds can reach) -
and the workgroups per CU the launch can hold (by its LDS)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK = 78.6e12
LDS_PER_CU = 160 * 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", type=int, default=37000)
    ap.add_argument("--segments", default="64,256,1024")
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    m = importlib.import_module("softgnss-python_amd")
    s = m.Settings()
    ctx = m.engine.get_context(s, 0)
    rec = ctx.synth(m.synth.Scene.default(), m.synth.record_length(s.samplesPerCode, a.ms))
    n = len(rec)
    _, copy_gbs = ctx.stream_rates()
    for N in (int(x) for x in a.segments.split(",")):
        J, S = m._native.excise_plan(n, N)
        M = N // 2
        ker = []
        for i in range(a.calls + 1):
            out, info = ctx.excise_record(rec, N, s.exciseThreshold, s.excisePasses)
            out.free()
            if i:
                ker.append(ctx.excise_timing())
        tiles = -(-(J - 1) // (S - 1))
        flops = 2.0 * 5.0 * M * np.log2(M) * tiles * S
        lds = 16 * 4096 + (S + 1) * M + 32 + 3584                   # the segments, the staged bytes, the small arrays
        print(json.dumps(dict(samples=n, segment=N, tile_segments=S, segments=J, calls=a.calls,
                              kernel_ms_min=round(min(ker), 3), kernel_ms_median=round(float(np.median(ker)), 3),
                              gsamples_per_s=round(n / (min(ker) * 1e-3) / 1e9, 2),
                              copy_gbs=round(copy_gbs, 1), copy_floor_ms=round(2.0 * n / (copy_gbs * 1e9) * 1e3, 3),
                              fp64_gflop=round(flops / 1e9, 1), fp64_floor_ms=round(flops / FP64_PEAK * 1e3, 3),
                              lds_bytes=lds, workgroups_per_cu=LDS_PER_CU // lds,
                              cells_cut=info["bins_cut"] / float(J * (M - 1)), clipped=info["clipped"])), flush=True)
    rec.free()


if __name__ == "__main__":
    main()
