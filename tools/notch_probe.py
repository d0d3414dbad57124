"""Time of sgx_if_filter's kernel (the interference-excision FIR, csrc/sgx_filter.hip) on one GPU:

    python tools/notch_probe.py [--ms 37000] [--taps 255,1025,4095] [--calls 10]

The record is the default scene of --ms code periods (37 000: the 1.4 GB record of the benchmark), the taps a notch at
IF + 180 kHz of each length.  One warm-up call, then --calls timed calls; HIP events on the context's stream around the
kernel.  Prints one JSON line per length: min and median in ms, and the multiply-accumulates per second they imply
(samples x taps; the padded taps the kernel also multiplies are not counted)."""
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
    ap.add_argument("--taps", default="255,1025,4095")
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    m = importlib.import_module("softgnss-python_amd")
    s = m.Settings()
    ctx = m.engine.get_context(s, 0)
    rec = ctx.synth(m.synth.Scene.default(), m.synth.record_length(s.samplesPerCode, a.ms))
    f = np.fft.rfftfreq(16384, 1e6 / s.samplingFreq)
    pxx = np.ones(f.size)
    pxx[int(round((s.IF + 180e3) / 1e6 / f[1]))] = 1e4          # one line, as the jammed scene of the tests has it
    for L in (int(x) for x in a.taps.split(",")):
        taps, shift, lines = m._native.notch_design(s, f, pxx, s.notchThresholdDb, s.notchWidthHz, L)
        ker = []
        for i in range(a.calls + 1):
            out = ctx.filter_record(rec, taps, shift)
            out.free()
            if i:
                ker.append(ctx.filter_timing())
        macs = float(len(rec)) * L
        print(json.dumps(dict(samples=len(rec), taps=L, lines=len(lines), calls=a.calls,
                              kernel_ms_min=round(min(ker), 3), kernel_ms_median=round(float(np.median(ker)), 3),
                              tera_macs_per_s=round(macs / (min(ker) * 1e-3) / 1e12, 2),
                              gsamples_per_s=round(len(rec) / (min(ker) * 1e-3) / 1e9, 2))), flush=True)
    rec.free()


if __name__ == "__main__":
    main()
