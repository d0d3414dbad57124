"""Time of sgx_if_from_iq's kernel (the I/Q -> real IF converter, csrc/sgx_iq.hip) on one GPU:

    python tools/iq_probe.py [--ms 37000] [--taps 31,63,255] [--calls 10]

The record is the default scene of --ms code periods (37 000: the 1.4 GB record of the benchmark), read as interleaved I/Q
bytes.  Per length: dense random taps without a zero (both polyphase branches at full length), and the designed half-band
filter (one branch is its single centre tap).  One warm-up call, then --calls timed calls; HIP events on the context's
stream around the kernel.  Prints one JSON line per filter - min and median in ms, the bytes read plus written per second
- after one line with the read and copy rates sgx_stream_rates measures on the same GPU: the copy rate is the floor for a
pass that reads N bytes and writes N bytes."""
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
    ap.add_argument("--taps", default="31,63,255")
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    m = importlib.import_module("softgnss-python_amd")
    s = m.Settings()
    ctx = m.engine.get_context(s, 0)
    n = m.synth.record_length(s.samplesPerCode, a.ms)
    rec = ctx.synth(m.synth.Scene.default(), n + n % 2)
    read_gbs, copy_gbs = ctx.stream_rates()
    print(json.dumps(dict(bytes=len(rec), read_GBps=round(read_gbs, 1), copy_GBps=round(copy_gbs, 1),
                          copy_floor_ms=round(2.0 * len(rec) / copy_gbs / 1e6, 3))), flush=True)
    rng = np.random.default_rng(1)
    for L in (int(x) for x in a.taps.split(",")):
        dense = rng.integers(1, 200, L).astype(np.int16) * rng.choice([-1, 1], L).astype(np.int16)
        for kind, (taps, shift) in (("dense", (dense, 12)), ("half-band", m._native.iq_design(L))):
            ker = []
            for i in range(a.calls + 1):
                out = ctx.iq_to_if(rec, taps, shift)
                out.free()
                if i:
                    ker.append(ctx.iq_timing())
            print(json.dumps(dict(taps=L, kind=kind, nonzero_taps=int(np.count_nonzero(taps)), calls=a.calls,
                                  kernel_ms_min=round(min(ker), 3), kernel_ms_median=round(float(np.median(ker)), 3),
                                  GBps_read_plus_written=round(2.0 * len(rec) / (min(ker) * 1e-3) / 1e9, 1),
                                  tera_macs_per_s=round(len(rec) * np.count_nonzero(taps) / 2.0 / (min(ker) * 1e-3) / 1e12, 2))),
                  flush=True)
    rec.free()


if __name__ == "__main__":
    main()
