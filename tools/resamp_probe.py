"""Times of the resampler's kernel (csrc/sgx_resamp.hip: sgx_if_resample) on one GPU beside the copy rate, and the comparison
the stage exists for: a 4.096 Msps capture processed directly and processed behind L = 10:

    python tools/resamp_probe.py [--out-bytes 1400000000] [--calls 10] [--gain-ms 2000] [--no-stage] [--no-gain]

One warm-up call, then --calls timed calls per configuration; HIP events on the context's stream around the kernel.  Prints
one JSON line with the read and copy rates sgx_stream_rates measures in the same job; then one line per (L, M, taps) on an
output of about --out-bytes: min and median in ms, the time of bytes read + written at the copy rate (the floor), the useful
multiply-accumulates (one per tap of a sub-filter: n_out taps / L), the rate they are done at, and the share of the floor the
kernel reaches.

Then (unless --no-gain) the default scene's eight satellites synthesised at 4.096 Msps with the IF at 1.0 MHz, --gain-ms
code periods plus the acquisition window: once as it is, once resampled by 10 / 1 to 40.96 Msps.  Per path one line: the
stage's kernel time, the 32-PRN acquisition (min and median of three calls after a warm-up), the 8 channels tracked in
latency mode per code period, and the tracking kernel the timing struct reports (4 trk_kernel_multi, 5 trk3_kernel)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ((10, 1, 0), (10, 1, 121), (10, 1, 1023), (8, 1, 0), (5, 1, 0), (2, 1, 0), (16, 1, 0), (7, 3, 0), (3, 2, 0),
           (16, 3, 0))      # (L, M, taps; 0: 24 L + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-bytes", type=int, default=1400000000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--gain-ms", type=int, default=2000, help="code periods tracked in the comparison")
    ap.add_argument("--no-stage", action="store_true")
    ap.add_argument("--no-gain", action="store_true")
    a = ap.parse_args()
    m = importlib.import_module("softgnss-python_amd")
    n = m._native
    fs, f_if = 4096000.0, 1000000.0
    s = m.Settings()
    s.samplingFreq, s.IF = fs, f_if
    ctx = m.engine.get_context(s, 0)
    scene = m.synth.Scene.default(fs, f_if)
    if not a.no_stage:
        read_gbs, copy_gbs = ctx.stream_rates()
        print(json.dumps(dict(read_GBps=round(read_gbs, 1), copy_GBps=round(copy_gbs, 1))), flush=True)
        for L, M, Lh in CONFIGS:
            n_in = a.out_bytes * M // L
            n_in -= n_in % (64 * M)
            rec = ctx.synth(scene, n_in)
            taps, shift, _ = n.resamp_design(fs, L, M, Lh)
            ms = []
            for i in range(a.calls + 1):
                out = ctx.resample(rec, taps, shift, L, M)
                n_out = len(out)
                out.free()
                if i:
                    ms.append(ctx.resamp_timing())
            rec.free()
            copy_ms = (n_in + n_out) / copy_gbs / 1e6
            macs = n_out * float(taps.size) / L
            print(json.dumps(dict(kernel="resamp_kernel", L=L, M=M, taps=int(taps.size), in_bytes=n_in, out_bytes=n_out,
                                  calls=a.calls, kernel_ms_min=round(min(ms), 3),
                                  kernel_ms_median=round(float(np.median(ms)), 3), copy_ms=round(copy_ms, 3),
                                  TMACps=round(macs / min(ms) / 1e9, 1), GBps=round((n_in + n_out) / min(ms) / 1e6, 1),
                                  share_of_copy_floor=round(copy_ms / min(ms), 3))), flush=True)
    if a.no_gain:
        return
    # what the stage buys: the 4.096 Msps scene beside itself at 10 / 1
    s10 = m.Settings()
    s10.samplingFreq, s10.IF, s10.resampleUp = fs, f_if, 10
    real = s10._prepared_settings()
    ctx10 = m.engine.get_context(real, 0)
    n_rec = m.synth.record_length(s.samplesPerCode, a.gain_ms)
    rec = ctx.synth(scene, n_rec)
    ctx.sync()
    taps, shift, info = s10._resamp_design()
    res = ctx10.resample(rec, taps, shift, 10, 1)         # (the resampled record belongs to the context that reads it)
    stage_ms = []
    for i in range(a.calls):
        ctx10.resample(rec, taps, shift, 10, 1).free()
        stage_ms.append(ctx10.resamp_timing())
    print(json.dumps(dict(record="4.096 Msps x 10 / 1", fs_out=info["fs_out"], in_bytes=n_rec, out_bytes=len(res),
                          clipped=res.clipped / float(len(res)), kernel_ms_min=round(min(stage_ms), 3),
                          kernel_ms_median=round(float(np.median(stage_ms)), 3))), flush=True)
    for name, c, st, r, stage in (("direct", ctx, s, rec, 0.0), ("behind 10 / 1", ctx10, real, res, min(stage_ms))):
        spc = st.samplesPerCode
        t_acq = []
        for i in range(4):
            acq = m.AcquisitionResult(st, device=0)
            acq.acquire(m.DeviceSignal(r, 0, 11 * spc))
            if i:
                t_acq.append(c.timing()["acquire_ms"])
        acq.preRun()
        ch8 = [(int(ch.PRN), float(ch.acquiredFreq), float(ch.codePhase)) for ch in acq.channels if int(ch.PRN)]
        ms = a.gain_ms - 20
        c.track(r, ch8, 50)
        t8 = []
        for i in range(3):
            c.track(r, ch8, ms)
            t8.append(c.timing()["track_ms"])
        print(json.dumps(dict(record=name, samplingFreq=st.samplingFreq, satellites=len(ch8), code_periods=ms,
                              stage_ms=round(stage, 3), fft_length=n.acquire_fft_length(spc),
                              acquire_ms_min=round(min(t_acq), 3), acquire_ms_median=round(float(np.median(t_acq)), 3),
                              track8_us_per_code_period=round(1e3 * min(t8) / ms, 3),
                              track8_ms=round(min(t8), 3), total_ms=round(stage + min(t_acq) + min(t8), 3),
                              track_kernel=int(c.timing()["track_kernel"]))), flush=True)
    res.free()
    rec.free()


if __name__ == "__main__":
    main()
